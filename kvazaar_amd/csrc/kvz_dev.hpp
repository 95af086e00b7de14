// kvz_dev.hpp -- device-resident batch kernels behind include/kvz_hip_dev.h.  Included by kvz_hip.hip.
//
// These are the HBM-streaming forms of the primitives: every byte of the inputs is read once with 8- or 16-byte loads
// that are contiguous across the lanes of a wavefront, the arithmetic happens in registers (v_sad_u8, packed int16
// Hadamard, MFMA), and one value per block goes back.  Rooflines: 2 n^2 bytes per SAD / SATD block,
// 4 n^2 bytes per transform block (+ 4 n^3 integer multiply-adds for the 16 / 32-point ones on the matrix cores).
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <mutex>
#include <chrono>
#include <vector>

#include "../../include/kvz_hip_dev.h"
#include "kvz_mfma.hpp"
#include "kvz_ops.hpp"
#include "kvz_sao.hpp"
#include "kvz_entropy.hpp"
#include "kvz_select.hpp"
#include "kvz_recon.hpp"
#include "kvz_tables.hpp"

namespace kvz {

// Sum over aligned groups of G consecutive lanes (G a power of two <= 64); the result is valid in the group's first lane.
__device__ __forceinline__ u32 load_u32_any(const u8 *p) { u32 v; __builtin_memcpy(&v, p, 4); return v; }  // any byte alignment
template <int G> __device__ __forceinline__ u32 group_sum(u32 v)
{
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_down(v, off, G);
  return v;
}

// ---------------------------------------------------------------------------------------------------------------
// SAD: one lane per 16 bytes of each input (dwordx4 loads, lane-contiguous), v_sad_u8 per dword, then a segmented sum
// over the n^2 / 16 lanes of a block.  64x64 blocks span four wavefronts: one atomic per wavefront into the zeroed output.
template <int N> __global__ void __launch_bounds__(256) dev_sad_kernel(const uint4 *a, const uint4 *b, const long chunks, u32 *out)
{
  constexpr int G = N * N / 16;  // lanes per block
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  u32 v = 0;
  if (i < chunks) {
    const uint4 x = a[i], y = b[i];
    v = __builtin_amdgcn_sad_u8(x.x, y.x, 0);
    v = __builtin_amdgcn_sad_u8(x.y, y.y, v);
    v = __builtin_amdgcn_sad_u8(x.z, y.z, v);
    v = __builtin_amdgcn_sad_u8(x.w, y.w, v);
  }
  if (G <= 64) {
    v = group_sum<(G <= 64 ? G : 64)>(v);
    if ((threadIdx.x & (G - 1)) == 0 && i < chunks) out[i / G] = v;
  } else {
    v = group_sum<64>(v);
    if ((threadIdx.x & 63) == 0 && i < chunks) atomicAdd(&out[i / G], v);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// SATD: one lane per 8x8 tile.  The lane reads its eight rows of both blocks as 8-byte loads (the lanes of a block row
// read consecutive addresses), forms the differences as packed int16 and runs the 8x8 Hadamard in registers: two packed
// stages along the rows, three down the columns, the last row stage folded into the magnitude sum
// (|p + q| + |p - q| = 2 max(|p|, |q|)).  Per tile (sum + 2) >> 2 (picture-generic.c:252-340), then the sum over the
// (n/8)^2 tiles of the block (strategies-picture.h:53-69).
typedef short dev_pk16 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32 dev_absmax(dev_pk16 a)
{
  const dev_pk16 m = __builtin_elementwise_max(a, -a);
  return (u32)imax((int)m.x, (int)m.y);
}
__device__ __forceinline__ void dev_diff_row(uint2 x, uint2 y, dev_pk16 *d)
{
  const u32 xs[2] = { x.x, x.y }, ys[2] = { y.x, y.y };
  for (int h = 0; h < 2; h++) {
    dev_pk16 lo, hi;
    lo.x = (short)((int)(xs[h] & 0xff) - (int)(ys[h] & 0xff));
    lo.y = (short)((int)((xs[h] >> 8) & 0xff) - (int)((ys[h] >> 8) & 0xff));
    hi.x = (short)((int)((xs[h] >> 16) & 0xff) - (int)((ys[h] >> 16) & 0xff));
    hi.y = (short)((int)(xs[h] >> 24) - (int)(ys[h] >> 24));
    d[2 * h] = lo; d[2 * h + 1] = hi;
  }
}
__device__ __forceinline__ u32 dev_satd8_regs(dev_pk16 d[8][4])
{
  for (int r = 0; r < 8; r++) {
    const dev_pk16 a0 = d[r][0] + d[r][2], a1 = d[r][1] + d[r][3], a2 = d[r][0] - d[r][2], a3 = d[r][1] - d[r][3];
    d[r][0] = a0 + a1; d[r][1] = a0 - a1; d[r][2] = a2 + a3; d[r][3] = a2 - a3;
  }
  u32 sum = 0;
  for (int j = 0; j < 4; j++) {
    const dev_pk16 a0 = d[0][j] + d[4][j], a1 = d[1][j] + d[5][j], a2 = d[2][j] + d[6][j], a3 = d[3][j] + d[7][j];
    const dev_pk16 a4 = d[0][j] - d[4][j], a5 = d[1][j] - d[5][j], a6 = d[2][j] - d[6][j], a7 = d[3][j] - d[7][j];
    const dev_pk16 b0 = a0 + a2, b1 = a1 + a3, b2 = a0 - a2, b3 = a1 - a3, b4 = a4 + a6, b5 = a5 + a7, b6 = a4 - a6, b7 = a5 - a7;
    sum += dev_absmax(b0 + b1) + dev_absmax(b0 - b1) + dev_absmax(b2 + b3) + dev_absmax(b2 - b3);
    sum += dev_absmax(b4 + b5) + dev_absmax(b4 - b5) + dev_absmax(b6 + b7) + dev_absmax(b6 - b7);
  }
  return 2 * sum;
}
template <int N> __global__ void __launch_bounds__(256) dev_satd_kernel(const u8 *a, const u8 *b, const long tiles, u32 *out)
{
  constexpr int TW = N / 8, T = TW * TW;  // tiles per block row / per block
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  u32 v = 0;
  if (t < tiles) {
    const long blk = t / T;
    const int tt = (int)(t % T), ty = tt / TW, tx = tt % TW;
    const long base = blk * (N * N) + (long)(ty * 8) * N + tx * 8;
    dev_pk16 d[8][4];
    for (int r = 0; r < 8; r++) {
      const uint2 x = *reinterpret_cast<const uint2 *>(a + base + r * N), y = *reinterpret_cast<const uint2 *>(b + base + r * N);
      dev_diff_row(x, y, d[r]);
    }
    v = (dev_satd8_regs(d) + 2) >> 2;
  }
  if (T <= 64) {
    v = group_sum<(T <= 64 ? T : 64)>(v);
    if ((threadIdx.x & (T - 1)) == 0 && t < tiles) out[t / T] = v;
  }
}
__global__ void __launch_bounds__(256) dev_satd4_kernel(const u8 *a, const u8 *b, const long blocks, u32 *out)
{
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= blocks) return;
  const uint4 x = reinterpret_cast<const uint4 *>(a)[i], y = reinterpret_cast<const uint4 *>(b)[i];
  u8 pa[16], pb[16];
  const u32 xs[4] = { x.x, x.y, x.z, x.w }, ys[4] = { y.x, y.y, y.z, y.w };
  for (int k = 0; k < 16; k++) { pa[k] = (u8)(xs[k >> 2] >> (8 * (k & 3))); pb[k] = (u8)(ys[k >> 2] >> (8 * (k & 3))); }
  out[i] = satd4(pa, 4, pb, 4);
}

// ---------------------------------------------------------------------------------------------------------------
// 16- and 32-point DCT / IDCT on the matrix cores: one wavefront per block, both passes chained through registers.
// With T the transform matrix (Tables::dct_i8, signed bytes) and X the n x n input:
//   forward: D0^T = X T^T, K = T D0^T   -> out = K       (dct-generic.c partial_butterfly_*, intermediate wraps to int16)
//   inverse: U = X^T T,    O = U^T T    -> out = O       (partial_butterfly_inverse_*, both stages clip to int16)
// The accumulator layout of v_mfma (lane = column, registers = 4 consecutive rows per k-step) is the B operand layout of
// the next product and, read as A, the transposed matrix, so the first result feeds the second product directly.
// Exactness: int8 operands, int32 accumulators (kvz_mfma.hpp): 16-bit values go in as a signed high and a biased low byte plane.
// Memory side: a wavefront moves its block between HBM and LDS with 16-byte accesses (2 KB per 32x32 block = two dwordx4 per lane) and feeds the
// matrix cores from LDS -- the operand layouts want 2-byte column gathers (inverse input) and 2-byte row scatters (every output), which cost
// 16 narrow global accesses per lane when done against HBM directly.
template <int N> __global__ void __launch_bounds__(256) dev_transform_mfma_kernel(const i16 *in, i16 *out, const int count, const int inverse, const Tables *tb)
{
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if constexpr (N == 16) {
    // FOUR blocks per wavefront (2 KB: two dwordx4 per lane each way); nothing is shared between wavefronts, so they synchronise on their own (a wavefront's LDS
    // operations execute in order: a compiler fence, no s_barrier), load the table operands once and run the four blocks' product chains side by side
    __shared__ alignas(16) i16 s_blk[4][4 * 256];
    i16 *sb = s_blk[wave];
    const long blk = ((long)blockIdx.x * 4 + wave) * 4;
    const long left = (long)count - blk;  // wavefront-uniform
    if (left <= 0) return;
    const uint4 *src = reinterpret_cast<const uint4 *>(in + blk * 256);
    uint4 *dst = reinterpret_cast<uint4 *>(out + blk * 256);
#pragma unroll
    for (int k = 0; k < 2; k++) { const int j = k * 64 + lane; if ((j >> 5) < left) reinterpret_cast<uint4 *>(sb)[j] = src[j]; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    mfma_transform_blocks16<4>(sb, sb, inverse != 0, tb, lane);  // (blocks past the end: whatever the LDS holds, never stored)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int k = 0; k < 2; k++) { const int j = k * 64 + lane; if ((j >> 5) < left) dst[j] = reinterpret_cast<const uint4 *>(sb)[j]; }
  } else {
    __shared__ alignas(16) i16 s_blk[4][N * N];
    const long blk = (long)blockIdx.x * 4 + wave;
    const bool have = blk < count;  // wavefront-uniform
    i16 *sb = s_blk[wave];
    if (have) { const uint4 *src = reinterpret_cast<const uint4 *>(in + blk * (N * N)); for (int k = 0; k < 2; k++) reinterpret_cast<uint4 *>(sb)[k * 64 + lane] = src[k * 64 + lane]; }
    __syncthreads();
    if (have) mfma_transform_block<N>(sb, sb, inverse != 0, tb, lane);
    __syncthreads();
    if (have) { uint4 *dst = reinterpret_cast<uint4 *>(out + blk * (N * N)); for (int k = 0; k < 2; k++) dst[k * 64 + lane] = reinterpret_cast<const uint4 *>(sb)[k * 64 + lane]; }
  }
}

// 4- and 8-point transforms (and the 4x4 DST) on the vector ALU, one lane per block ROW: a row of int16 arrives as packed pairs (one 8- or
// 16-byte load, lane-contiguous), an output is NB / 2 v_dot2_i32_i16 against pairs of matrix entries held in scalar registers with the
// rounding constant as the initial accumulator; the transposition between (and after / before) the two passes goes through a padded LDS tile:
// NB 2-byte writes, one 8- or 16-byte read per row.  forward (dct-generic.c:559-579): pass, transpose, pass, transpose; inverse: transpose, pass,
// transpose, pass.  Four rows per lane (loads of all four in flight at once), 1024 rows per workgroup.
template <int NB> __global__ void __launch_bounds__(256) dev_transform_rows_kernel(const i16 *in, i16 *out, const long rows_total, const int inverse, const u32 *pairs /* [2][NB][NB / 2], rows padded to 4 pairs for NB = 4 */)
{
  constexpr int R = NB == 16 ? 2 : 4, PW = NB / 2, KS = NB == 16 ? 8 : 4, WS = NB == 16 ? 128 : 32, BS = NB * NB + (NB == 4 ? 4 : 8), BLOCKS = R * 256 / NB, L2 = NB == 4 ? 2 : (NB == 8 ? 3 : 4);
  typedef short s16x2 __attribute__((ext_vector_type(2)));
  __shared__ alignas(16) i16 s_t[BLOCKS * BS];
  const int tid = threadIdx.x;
  const u32 *cp = pairs + (inverse ? WS : 0);  // uniform: the matrix pairs come through the scalar cache (this table is never rewritten)
  u32 p[R][PW];
  long row[R];
  int base[R];  // element offset of the row's block in the tile
  const int r = tid % NB;  // the row's index in its block (256 is a multiple of NB: the same for every row of the lane)
  auto rd = [&](const i16 *ptr, u32 *x) {  // one row = PW dwords
    if (NB == 4) { const uint2 v = *reinterpret_cast<const uint2 *>(ptr); x[0] = v.x; x[1] = v.y; }
    else for (int h = 0; h < PW / 4; h++) { const uint4 v = reinterpret_cast<const uint4 *>(ptr)[h]; x[4 * h] = v.x; x[4 * h + 1] = v.y; x[4 * h + 2] = v.z; x[4 * h + 3] = v.w; }
  };
  auto wr = [&](i16 *ptr, const u32 *x) {
    if (NB == 4) *reinterpret_cast<uint2 *>(ptr) = make_uint2(x[0], x[1]);
    else for (int h = 0; h < PW / 4; h++) reinterpret_cast<uint4 *>(ptr)[h] = make_uint4(x[4 * h], x[4 * h + 1], x[4 * h + 2], x[4 * h + 3]);
  };
#pragma unroll
  for (int q = 0; q < R; q++) {
    row[q] = ((long)blockIdx.x * R + q) * 256 + tid;
    base[q] = ((q * 256 + tid) / NB) * BS;
    for (int i = 0; i < PW; i++) p[q][i] = 0;
    if (row[q] < rows_total) rd(in + row[q] * NB, p[q]);
  }
  auto pass = [&](const u32 *x, int shift, bool clip, int *y) {
#pragma unroll
    for (int k = 0; k < NB; k++) {
      int acc = 1 << (shift - 1);
#pragma unroll
      for (int i = 0; i < PW; i++) acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, x[i]), __builtin_bit_cast(s16x2, cp[k * KS + i]), acc, false);
      acc >>= shift;
      y[k] = clip ? iclip(-32768, 32767, acc) : acc;
    }
  };
  auto put = [&](int q, const int *y) {  // element e of the lane's row -> [e][row]
#pragma unroll
    for (int e = 0; e < NB; e++) s_t[base[q] + e * NB + r] = (i16)y[e];
  };
  auto get = [&](int q, u32 *x) { rd(&s_t[base[q] + r * NB], x); };  // the lane's row of the tile
  int y[NB];
  if (!inverse) {
#pragma unroll
    for (int q = 0; q < R; q++) { pass(p[q], L2 - 1, false, y); put(q, y); }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < R; q++) get(q, p[q]);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < R; q++) { pass(p[q], L2 + 6, false, y); put(q, y); }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < R; q++) get(q, p[q]);
  } else {
#pragma unroll
    for (int q = 0; q < R; q++) { for (int e = 0; e < NB; e++) y[e] = (int)(i16)(p[q][e >> 1] >> (16 * (e & 1))); put(q, y); }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < R; q++) get(q, p[q]);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < R; q++) { pass(p[q], 7, true, y); put(q, y); }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < R; q++) {
      u32 x[PW];
      get(q, x);
      pass(x, 12, true, y);
      for (int i = 0; i < PW; i++) p[q][i] = __builtin_amdgcn_perm((u32)y[2 * i + 1], (u32)y[2 * i], 0x05040100u);
    }
  }
#pragma unroll
  for (int q = 0; q < R; q++)
    if (row[q] < rows_total) wr(out + row[q] * NB, p[q]);
}

// 4- and 8-point transforms (and the 4x4 DST): 16 / n blocks sit on the diagonal of one 16x16 problem, the matrix is the
// matching block-diagonal one (Tables::bd_i8), everything else as above.  Off-diagonal results are exact zeros and never stored.
template <int NB /* block size: 4 or 8 */> __global__ void __launch_bounds__(256)
dev_transform_small_mfma_kernel(const i16 *in, i16 *out, const int count, const int inverse, const int8_t *T, const int8_t *Tt, const i32 *sT, const i32 *sTt)
{
  typedef DevMma<16> M;
  constexpr int L2 = NB == 4 ? 2 : 3, G = 16 / NB;
  const int lane = threadIdx.x & 63;
  const long first = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * G;  // first block of this wavefront
  if (first >= count) return;  // wavefront-uniform
  const int col = M::idx(lane), g = col / NB, cc = col - g * NB, k0 = M::k0(lane, 0);
  const bool have = first + g < count;          // the lane's own block exists
  const bool diag = k0 / NB == g;               // the lane's four k lie in its block
  const i16 *x = in + (first + g) * (NB * NB);
  i16 *o = out + (first + g) * (NB * NB);
  int v[4], t[4];
  for (int i = 0; i < 4; i++) {
    const int kk = k0 - g * NB + i;
    v[i] = (have && diag) ? (int)(inverse ? x[kk * NB + cc] : x[cc * NB + kk]) : 0;
  }
  if (!inverse) {
    dev_product<16>(v, T, sT, false, lane, 1 << (L2 - 2), t);
    for (int r = 0; r < 4; r++) v[r] = t[r] >> (L2 - 1);
    dev_product<16>(v, T, sT, true, lane, 1 << (L2 + 5), t);
    for (int r = 0; r < 4; r++) v[r] = t[r] >> (L2 + 6);
  } else {
    dev_product<16>(v, Tt, sTt, false, lane, 64, t);
    for (int r = 0; r < 4; r++) v[r] = iclip(-32768, 32767, t[r] >> 7);
    dev_product<16>(v, Tt, sTt, false, lane, 2048, t);
    for (int r = 0; r < 4; r++) v[r] = iclip(-32768, 32767, t[r] >> 12);
  }
  for (int r = 0; r < 4; r++) {
    const int row = M::row(lane, r);
    if (have && row / NB == g) o[(row - g * NB) * NB + cc] = (i16)v[r];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Angular prediction of a batch of blocks with one mode (intra-generic.c:49-155), row-wise: a lane produces groups of 4 horizontally
// adjacent samples of the *vertical* problem -- for modes >= 18 that is the block itself, for modes < 18 the block with the references
// swapped and the result transposed.  Along a row the displacement (delta_int, delta_fract) is one number, so a group needs 5 consecutive
// bytes of the main reference: two aligned LDS dwords funnel-shifted into place, then the two-tap interpolation on two samples per 32-bit
// multiply (the 16-bit halves cannot carry: (32 - f) a + f b + 16 <= 8176).  Horizontal modes: the four lanes of a quad hold the same four
// columns of four consecutive rows; they exchange their dwords by DPP (quad_perm broadcasts), each picks one byte column (v_perm_b32) and
// holds four horizontally adjacent samples of the transposed block, which go through an LDS tile as dwords to be stored lane-contiguously.
// A workgroup stages the references of its blocks (one contiguous byte range per side, copied as dwords whatever its alignment); modes with
// a negative angle first build each block's extended main reference ext[k + W] = ref_main[k], k = -W .. W, the negative indices projected
// from the side reference (intra-generic.c:82-104); the others read the staged bytes directly.
// Bytes per block: 2 (2 W + 1) read, W^2 written.
constexpr int kAngularGroupsPerLane = 8;  // 2048 groups = 8 KB of output per workgroup: enough bytes in flight per barrier phase to cover the load latency
// kvz_hip_dev_intra_select: the CTU pass's selection (select_on_wave) on tables in memory, a wavefront per table -- lane m brings mode m's SATD and cost as
// CtuProgramT::replay_selection does from LDS
__global__ void __launch_bounds__(256) dev_intra_select_kernel(const u32 *raw, const int8_t *preds, const double *mode_bits, const int count, const int log2w, const int nblk,
                                                               int32_t *winner)
{
  const long table = (long)blockIdx.x * 4 + (threadIdx.x >> 6);  // wavefront-uniform: all 64 lanes stay or leave together
  if (table >= count) return;
  const int lane = threadIdx.x & 63, my_mode = lane < 35 ? lane : 0;
  const int p0 = preds[3 * table], p1 = preds[3 * table + 1], p2 = preds[3 * table + 2];
  const double bits[3] = { mode_bits[3 * table], mode_bits[3 * table + 1], mode_bits[3 * table + 2] };
  const u32 my_raw = select_satd_sum(raw + (table * 35 + my_mode) * nblk, nblk);
  const int w = select_on_wave(lane, my_raw, select_mode_cost(my_raw, my_mode, p0, p1, p2, bits), p0, p1, p2, log2w);
  if (lane == 0) winner[table] = w;
}

// kvz_hip_dev_cu8_units: stages 2-5 of the CTU pass's 8x8 CU (kvz_recon.hpp cu8_*: what kvz_ctu.hpp recon_cu8 calls) on units in memory, two wavefronts
// per unit with recon_cu8's roles: threads 0..63 the luma samples, 64..79 / 80..95 the U / V samples.  A unit: Y 64 | U 16 | V 16 int16, row-major.
struct Cu8MatRow { u32 w[4]; };
template <int L2> KVZ_DEV void dev_cu8_lane(int stage, int c, int e, i16 (*t)[96], int from_coeffs, int qp, const Cu8MatRow &fwd, const Cu8MatRow &inv, const i16 *in, i16 *levels, i16 *dequant,
                                            i16 *resid)
{
  const int po = c == 0 ? 0 : (c == 1 ? 64 : 80);
  i16 *t0 = t[0] + po, *t1 = t[1] + po;
  if (stage == 1) { if (!from_coeffs) t0[e] = in[po + e]; }
  else if (stage == 2) { if (!from_coeffs) t1[e] = cu8_fwd_first<L2>(t0, e, fwd); }
  else if (stage == 3) {
    int level = 0, dq = in[po + e];
    if (!from_coeffs) {
      const QuantScalars q = quant_scalars(qp, 8, 1, 0, 1 << L2, c ? 2 : 0);
      level = quant_level(cu8_fwd_second<L2>(t1, e, fwd), q);
      dq = dequant_level(level, q);
    }
    levels[po + e] = (i16)level;
    dequant[po + e] = (i16)dq;
    t0[cu8_transposed<L2>(e)] = (i16)dq;
  }
  else if (stage == 4) t1[cu8_transposed<L2>(e)] = cu8_inv_first<L2>(t0, e, inv);
  else resid[po + e] = cu8_inv_second<L2>(t1, e, inv);
}
__global__ void __launch_bounds__(256) dev_cu8_units_kernel(const i16 *in, const int32_t *qp, const int count, const int from_coeffs, const Tables *tb, i16 *levels, i16 *dequant, i16 *resid)
{
  __shared__ alignas(16) i16 t[2][2][96];  // two units per workgroup, each on its own pair of wavefronts
  const int half = threadIdx.x >> 7, tid = threadIdx.x & 127;
  const long unit = 2l * blockIdx.x + half, o = 96 * unit;
  const bool live = unit < count && tid < 96;  // (every thread stays for the barriers)
  const int c = tid < 64 ? 0 : (tid < 80 ? 1 : 2), e = tid < 64 ? tid : (tid & 15), q = live ? qp[unit] : 0;
  Cu8MatRow fwd = {}, inv = {};
  if (tid < 64) cu8_matrix_rows<3>(tb, e, fwd, inv); else cu8_matrix_rows<2>(tb, e, fwd, inv);
  for (int stage = 1; stage <= 5; stage++) {
    if (live) {
      if (tid < 64) dev_cu8_lane<3>(stage, c, e, t[half], from_coeffs, q, fwd, inv, in + o, levels + o, dequant + o, resid + o);
      else dev_cu8_lane<2>(stage, c, e, t[half], from_coeffs, q, fwd, inv, in + o, levels + o, dequant + o, resid + o);
    }
    __syncthreads();
  }
}

// kvz_hip_dev_satd8_blocks: the rough search's group routine (kvz_mfma.hpp satd8_group_mfma: what kvz_ctu.hpp angular_group_satd calls) on pairs of 8x8 byte blocks
// in memory, a wavefront per 32 pairs
__global__ void __launch_bounds__(256) dev_satd8_blocks_kernel(const Tables *tb, const u8 *a, const u8 *b, const int count, u32 *out)
{
  dev_satd8_blocks_wave(tb, a, b, count, out, (int)(blockIdx.x * 4 + (threadIdx.x >> 6)), (int)(threadIdx.x & 63));
}

// kvz_hip_dev_rough_rows: what the rough search of an 8x8 / 16x16 CU predicts for modes 2..33, from unfiltered references in memory: the pass's own reference filter
// (luma_filtered_ref), extended references (Tables::mref_tab, mref_copy), edge bytes (satd_edge_byte) and row generator (Tables::satd_rows, satd_rows_predict) on an
// LDS image laid out like CtuShared from its `ref` on, two wavefronts per CU in the pass's roles (an 8x8 CU's group on the first; groups 2 t, 2 t + 1 of a 16x16 CU
// on wavefront t).  The generator's rows run across the main reference: a horizontal mode's block comes out transposed and is written back upright.
template <int L2> __global__ void __launch_bounds__(256) dev_rough_rows_kernel(const Tables *tb, const u8 *top, const u8 *left, const int count, u8 *out)
{
  constexpr int W = 1 << L2, N = 2 * W + 1, NM = (15 * (2 * W + 2) + 127) / 128, LB = 2 * (L2 - 3), NBLK = 1 << LB;
  static_assert(2 * N <= 128 && NM * 128 <= 512, "a lane per reference sample; Tables::mref_tab rows");
  __shared__ alignas(16) u8 lds[2][(kSatdEdge + 1 + 2 * 16 + 15) & ~15u];  // two CUs per workgroup, each on its own pair of wavefronts
  const int half = threadIdx.x >> 7, tid = threadIdx.x & 127, lane = tid & 63;
  const long cu = 2l * blockIdx.x + half;
  const bool live = cu < count;  // (every thread stays for the barriers)
  u8 *ref0 = lds[half];
  const int side = tid >= N, k = side ? tid - N : tid;
  if (live && tid < 2 * N) ref0[kMrefRefRow * side + k] = (side ? left : top)[cu * N + k];
  __syncthreads();
  if (live && tid < 2 * N) ref0[kMrefFiltered + kMrefRefRow * side + k] = luma_filtered_ref(ref0, N, tid);
  __syncthreads();
  if (live) {
    u32 e[NM];
    for (int j = 0; j < NM; j++) e[j] = tb->mref_tab[L2 - 3][tid + j * 128];
    mref_copy<NM>(ref0, e);
    if (tid <= 2 * W) {
      const u8 xv = satd_edge_byte(ref0, L2, tid & (2 * W - 1));
      ref0[kSatdEdge + (tid == 2 * W ? 0 : 1 + tid)] = tid == 2 * W ? (u8)0 : xv;
    }
  }
  __syncthreads();
  if (!live || (L2 == 3 && tid >= 64)) return;
#pragma unroll
  for (int j = 0; j < (L2 == 4 ? 2 : 1); j++) {
    const int g = L2 == 4 ? 2 * (tid >> 6) + j : 0, pr = 32 * g + (lane & 31), mode = 2 + (pr >> LB), b = pr & (NBLK - 1);
    const dev_int4 *row = reinterpret_cast<const dev_int4 *>(tb->satd_rows[L2 == 4 ? 1 + g : 0][lane]);
    const dev_int4 e[2] = { row[0], row[1] };
    dev_int4 p[2];
    satd_rows_predict(ref0, e, p);
    u8 *o = out + ((cu * 32 + (mode - 2)) * NBLK + b) * 64;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int x = 0; x < 8; x++) {
        const int r = 4 * (lane >> 5) + i;
        const u8 v = (u8)(((u32)p[i >> 1][2 * (i & 1) + (x >> 2)] >> (8 * (x & 3))) ^ 0x80);
        o[mode >= 18 ? 8 * r + x : 8 * x + r] = v;
      }
  }
}

// kvz_hip_dev_cu16_predict: stage 1's luma prediction of a 16x16 CU's reconstruction (kvz_ctu.hpp recon_cu16) from unfiltered references in memory, a mode per CU:
// the pass's reference filter and extended references as above, two wavefronts per CU, then the first one predicts in recon_cu16's lane roles -- lane = row segment
// of four samples (kvz_recon.hpp cu16_predict_lane), one 4-byte store each.
__global__ void __launch_bounds__(256) dev_cu16_predict_kernel(const Tables *tb, const u8 *top, const u8 *left, const u8 *modes, const int count, u8 *out)
{
  constexpr int W = 16, N = 2 * W + 1, NM = (15 * (2 * W + 2) + 127) / 128;
  static_assert(2 * N <= 128 && NM * 128 <= 512, "a lane per reference sample; Tables::mref_tab rows");
  __shared__ alignas(16) u8 lds[2][(kMrefExtended + 15 * kMrefStride + 15) & ~15u];  // two CUs per workgroup, each on its own pair of wavefronts
  const int half = threadIdx.x >> 7, tid = threadIdx.x & 127;
  const long cu = 2l * blockIdx.x + half;
  const bool live = cu < count;  // (every thread stays for the barriers)
  u8 *ref0 = lds[half];
  const int side = tid >= N, k = side ? tid - N : tid;
  if (live && tid < 2 * N) ref0[kMrefRefRow * side + k] = (side ? left : top)[cu * N + k];
  __syncthreads();
  if (live && tid < 2 * N) ref0[kMrefFiltered + kMrefRefRow * side + k] = luma_filtered_ref(ref0, N, tid);
  __syncthreads();
  if (live) {
    u32 e[NM];
    for (int j = 0; j < NM; j++) e[j] = tb->mref_tab[1][tid + j * 128];
    mref_copy<NM>(ref0, e);
  }
  __syncthreads();
  if (!live || tid >= 64) return;
  const int mode = imin(modes[cu], 34);  // (a mode that does not exist reads nothing out of bounds)
  int disp, inv;
  angular_params(mode, &disp, &inv);
  alignas(4) u8 p[4];
  cu16_predict_lane(ref0, mode, dc_value(4, ref0, ref0 + kMrefRefRow), disp, inv, tid, p);
  __builtin_memcpy(__builtin_assume_aligned(out + cu * (W * W) + 4 * tid, 4), p, 4);
}

template <int L2> __global__ void __launch_bounds__(256) dev_angular_kernel(const u8 *above, const u8 *left, const int count, const int mode, u8 *out)
{
  constexpr int W = 1 << L2, NG = kAngularGroupsPerLane, GPB = W * W / 4, BLOCKS = 256 * NG / GPB, RS = 2 * W + 1, ES = (2 * W + 1 + 8 + 3) & ~3;
  constexpr int RAW = (BLOCKS * RS + 3 + 3) / 4 + 2;
  __shared__ u32 s_raw[2][RAW];
  __shared__ alignas(8) u8 s_ext[BLOCKS][ES];
  __shared__ u32 s_tile[BLOCKS * W * W / 4];
  const int disp_tab[9] = { 0, 2, 5, 9, 13, 17, 21, 26, 32 };
  const int inv_tab[9] = { 0, 4096, 1638, 910, 630, 482, 390, 315, 256 };
  const bool vertical = mode >= 18;
  const int mode_disp = vertical ? mode - 26 : 10 - mode, ad = iabs(mode_disp);
  const int disp = mode_disp < 0 ? -disp_tab[ad] : disp_tab[ad], inv = inv_tab[ad];
  const long blk0 = (long)blockIdx.x * BLOCKS;
  const int nblk = (int)(count - blk0 < BLOCKS ? count - blk0 : BLOCKS);
  const long g0 = blk0 * RS;
  const int mis = (int)(g0 & 3), ndw = (mis + nblk * RS + 3) >> 2;
  const u8 *main_g = vertical ? above : left, *side_g = vertical ? left : above;
  const int tid = threadIdx.x;
  for (int i = tid; i < ndw; i += 256) {
    s_raw[0][i] = reinterpret_cast<const u32 *>(main_g + g0 - mis)[i];
    if (disp < 0) s_raw[1][i] = reinterpret_cast<const u32 *>(side_g + g0 - mis)[i];
  }
  __syncthreads();
  if (disp < 0) {
    const int lowest = (W * disp) >> 5, span = W + 1 - lowest;  // indices lowest .. W in use
    const u8 *rm = reinterpret_cast<const u8 *>(s_raw[0]) + mis, *rs = reinterpret_cast<const u8 *>(s_raw[1]) + mis;
    constexpr int LPB = BLOCKS >= 256 ? 1 : 256 / BLOCKS;  // lanes per block (no division by the run-time span)
    for (int bb = tid / LPB; bb < nblk; bb += 256 / LPB)
      for (int j = tid % LPB; j < span; j += LPB) {
        const int k = j + lowest;
        s_ext[bb][k + W] = k >= -1 ? rm[bb * RS + k + 1] : rs[bb * RS + ((128 + (-1 - k) * inv) >> 8)];
      }
    __syncthreads();
  }
  u32 *out32 = reinterpret_cast<u32 *>(out + blk0 * (W * W));
#pragma unroll
  for (int g = 0; g < NG; g++) {
    const int vl = tid + 256 * g, b = vl / GPB, q = vl % GPB;
    const int py = vertical ? q / (W / 4) : q % W, px = 4 * (vertical ? q % (W / 4) : q / W);
    // ref_main[k] = base[bo + k], base 4-byte aligned
    const u8 *base = disp < 0 ? &s_ext[b][0] : reinterpret_cast<const u8 *>(s_raw[0]);
    const int bo = disp < 0 ? W : mis + b * RS + 1;
    const int delta = (py + 1) * disp, di = delta >> 5;
    const u32 f = (u32)(delta & 31), c = 32 - f;
    const int j0 = bo + px + di, o = j0 & 3;
    const u32 *src = reinterpret_cast<const u32 *>(base + (j0 & ~3));
    const unsigned long long w = (((unsigned long long)src[1] << 32) | src[0]) >> (8 * o);
    const u32 A = (u32)w, B = (u32)(w >> 8);  // samples k and k + 1
    const u32 ev = (((A & 0x00ff00ffu) * c + (B & 0x00ff00ffu) * f + 0x00100010u) >> 5) & 0x00ff00ffu;
    const u32 od = ((((A >> 8) & 0x00ff00ffu) * c + ((B >> 8) & 0x00ff00ffu) * f + 0x00100010u) >> 5) & 0x00ff00ffu;
    const u32 res = ev | (od << 8);
    if (vertical) {
      if (b < nblk) out32[vl] = res;
    } else {
      // res = samples (px .. px + 3, py) of the vertical problem = out(x = py, y = px .. px + 3); the quad holds py & ~3 .. + 3
      const int r = (int)res, i = tid & 3;
      const u32 r0 = (u32)__builtin_amdgcn_update_dpp(0, r, 0x00, 0xf, 0xf, false), r1 = (u32)__builtin_amdgcn_update_dpp(0, r, 0x55, 0xf, 0xf, false);
      const u32 r2 = (u32)__builtin_amdgcn_update_dpp(0, r, 0xaa, 0xf, 0xf, false), r3 = (u32)__builtin_amdgcn_update_dpp(0, r, 0xff, 0xf, 0xf, false);
      const u32 sel = 0x0400u + (u32)i * 0x0101u;  // byte i of the low operand, byte i of the high one
      const u32 t01 = __builtin_amdgcn_perm(r1, r0, sel), t23 = __builtin_amdgcn_perm(r3, r2, sel);
      s_tile[(b * (W * W) + (px + i) * W + (py & ~3)) >> 2] = __builtin_amdgcn_perm(t23, t01, 0x05040100u);  // out(y = px + i, x = py & ~3 .. + 3)
    }
  }
  if (!vertical) {
    __syncthreads();
#pragma unroll
    for (int g = 0; g < NG; g++) {
      const int vl = tid + 256 * g;
      if (vl / GPB < nblk) out32[vl] = s_tile[vl];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Integer-pel motion cost surface: SAD of one BW x BW block of the current picture against the reference at every
// displacement of a (2 range + 1)^2 window -- kvz_image_calc_sad (image.c:407) per candidate, i.e. the reference is
// edge-replicated outside the frame (image.c:279-397).  One workgroup per block: the block and the (BW + 2 range)^2 window are
// staged in LDS once (clamped addressing does the replication), then a lane scores FOUR horizontally adjacent candidates at a time with
// v_qsad_pk_u16_u8: one instruction takes 8 window bytes and 4 block bytes and adds the SADs at byte offsets 0, 1, 2, 3 to four packed
// 16-bit sums -- 16 absolute differences per instruction, and the candidate's column needs no shifting into place.  The 16-bit sums are
// flushed into 32-bit ones every 256 / BW rows (256 / BW * BW * 255 < 65 536).  Window re-use between candidates never touches HBM again.
constexpr int kSadSurfaceLanes = 320;  // five wavefronts: the 33 x 9 = 297 groups of a +-16 search fit one round
template <int BW> __global__ void __launch_bounds__(kSadSurfaceLanes)
dev_sad_surface_kernel(const u8 *cur, const u8 *ref, const int W, const int H, const int range, const i16 *blk_xy, u32 *out)
{
  constexpr int MAXR = 32, WD = (BW + 2 * MAXR + 8) / 4;  // dwords per staged window row (+ the bytes a partial last group of four reads)
  constexpr int FL = 256 / BW >= BW ? BW : 256 / BW;       // rows per flush of the 16-bit sums
  constexpr int NT = kSadSurfaceLanes;
  __shared__ u32 s_cur[BW * BW / 4];
  __shared__ alignas(8) u32 s_win[(BW + 2 * MAXR) * WD];
  const int b = blockIdx.x, bx = blk_xy[2 * b], by = blk_xy[2 * b + 1], side = 2 * range + 1, wrows = BW + 2 * range, wcols = BW + 2 * range;
  u8 *win8 = reinterpret_cast<u8 *>(s_win);
  for (int i = threadIdx.x; i < BW * BW / 4; i += NT) s_cur[i] = load_u32_any(cur + (long)(by + i / (BW / 4)) * W + bx + 4 * (i % (BW / 4)));
  const int wdw = (wcols + 3) >> 2;  // dwords of a window row that hold samples
  if (bx - range >= 0 && bx - range + 4 * wdw <= W && by - range >= 0 && by - range + wrows <= H) {  // the window lies inside the picture: dword copies
    for (int i = threadIdx.x; i < wrows * wdw; i += NT) {
      const int r = i / wdw, c = i - r * wdw;
      s_win[r * WD + c] = load_u32_any(ref + (long)(by - range + r) * W + bx - range + 4 * c);
    }
  } else {
    for (int i = threadIdx.x; i < wrows * wcols; i += NT) {
      const int r = i / wcols, c = i % wcols;
      const int y = iclip(0, H - 1, by - range + r), x = iclip(0, W - 1, bx - range + c);
      win8[r * (WD * 4) + c] = ref[(long)y * W + x];
    }
  }
  __syncthreads();
  const int groups = (side + 3) >> 2;  // groups of four candidates along x
  for (int t = threadIdx.x; t < side * groups; t += NT) {
    const int dy = t / groups, d0 = t - dy * groups;  // window-relative displacement: row dy, columns 4 d0 .. 4 d0 + 3
    u32 sad[4] = { 0, 0, 0, 0 };
    for (int r0 = 0; r0 < BW; r0 += FL) {
      unsigned long long acc = 0;
#pragma unroll 4
      for (int r = r0; r < r0 + FL; r++) {
        const u32 *wr = s_win + (dy + r) * WD + d0;
        u32 lo = wr[0];
#pragma unroll
        for (int k = 0; k < BW / 4; k++) {
          const u32 hi = wr[k + 1];
          acc = __builtin_amdgcn_qsad_pk_u16_u8(((unsigned long long)hi << 32) | lo, s_cur[r * (BW / 4) + k], acc);
          lo = hi;
        }
      }
      for (int i = 0; i < 4; i++) sad[i] += (u32)(acc >> (16 * i)) & 0xffffu;
    }
    for (int i = 0; i < 4; i++)
      if (4 * d0 + i < side) out[(long)b * side * side + dy * side + 4 * d0 + i] = sad[i];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// SAO applied to whole pictures (kvz_sao_reconstruct, sao.c:302-361, for every CTU and plane): out = in + offset[category], the
// category from the sample and its two neighbours along the CTU's edge class, or from its band (sao-generic.c:84-124).
// Neighbours always come from `in` (the deblocked picture); samples whose neighbour would lie outside the picture keep their
// value (sao.c:324-349).  One lane per 4 samples of a plane row: dword load of the centre, byte loads of the six outer
// neighbours it does not already hold, dword store; one workgroup per plane row.
// Per (frame, CTU, plane) parameter record in 8 bytes: type | class | band position | offsets[0..4]
// One wavefront per CTU (blockIdx = group of four CTU columns | CTU row | frame).  Sixteen samples per lane, two per 32-bit operation: the bytes of the centre dword and of the two neighbour
// dwords (unaligned loads at the class's displacement) are spread over 16-bit halves (even / odd bytes), sign(c - n) + 1 = clamp(c + 1 - n, 0, 2)
// is three packed instructions per neighbour and pair, and the category -> offset table of the CTU's record is applied to all four samples by
// two v_perm_b32 (byte look-ups); band offsets use the same look-up on clamp(band - position + 1, 0, 5).
__device__ __forceinline__ u32 sao_add_offsets(u32 c4, u32 off4)  // clip(c + (int8)off) on four bytes
{
  const dev_pk16 ce = __builtin_bit_cast(dev_pk16, c4 & 0x00ff00ffu), co = __builtin_bit_cast(dev_pk16, (c4 >> 8) & 0x00ff00ffu);
  const dev_pk16 oe = __builtin_bit_cast(dev_pk16, off4 << 8) >> 8, oo = __builtin_bit_cast(dev_pk16, off4) >> 8;  // sign-extended int8 per half (even: the cross-half bits shifted in are shifted out again)
  const dev_pk16 lo = { 0, 0 }, hi = { 255, 255 };
  const dev_pk16 re = __builtin_elementwise_min(__builtin_elementwise_max(ce + oe, lo), hi), ro = __builtin_elementwise_min(__builtin_elementwise_max(co + oo, lo), hi);
  return __builtin_bit_cast(u32, re) | (__builtin_bit_cast(u32, ro) << 8);
}
__device__ __forceinline__ u32 sao_sign_idx(u32 c4, u32 a4, u32 b4)  // per byte: 2 + sign(c - a) + sign(c - b)
{
  const dev_pk16 one = { 1, 1 }, lo = { 0, 0 }, two = { 2, 2 };
  const dev_pk16 ce = __builtin_bit_cast(dev_pk16, c4 & 0x00ff00ffu) + one, co = __builtin_bit_cast(dev_pk16, (c4 >> 8) & 0x00ff00ffu) + one;
  auto sg = [&](dev_pk16 c1, u32 n) { return __builtin_elementwise_min(__builtin_elementwise_max(c1 - __builtin_bit_cast(dev_pk16, n), lo), two); };
  const dev_pk16 ie = sg(ce, a4 & 0x00ff00ffu) + sg(ce, b4 & 0x00ff00ffu), io = sg(co, (a4 >> 8) & 0x00ff00ffu) + sg(co, (b4 >> 8) & 0x00ff00ffu);
  return __builtin_bit_cast(u32, ie) | (__builtin_bit_cast(u32, io) << 8);
}
// 128-bit helpers: four dwords = sixteen samples
__device__ __forceinline__ uint4 load_u128_any(const u8 *p) { uint4 v; __builtin_memcpy(&v, p, 16); return v; }
__device__ __forceinline__ uint4 shl8_u128(uint4 v)  // byte k <- byte k - 1
{
  return make_uint4(v.x << 8, __builtin_amdgcn_alignbyte(v.y, v.x, 3), __builtin_amdgcn_alignbyte(v.z, v.y, 3), __builtin_amdgcn_alignbyte(v.w, v.z, 3));
}
__device__ __forceinline__ uint4 shr8_u128(uint4 v)  // byte k <- byte k + 1
{
  return make_uint4(__builtin_amdgcn_alignbyte(v.y, v.x, 1), __builtin_amdgcn_alignbyte(v.z, v.y, 1), __builtin_amdgcn_alignbyte(v.w, v.z, 1), v.w >> 8);
}
// TAIL: plane widths that are not multiples of 16 (the last lane of a row then holds 4, 8 or 12 samples, moved as single dwords)
template <bool TAIL> __global__ void __launch_bounds__(256) dev_sao_kernel(const u8 *in, u8 *out, const int W, const int H, const unsigned long long *packed, const kvz_hip_sao_params *luma,
                                                                          const kvz_hip_sao_params *chroma)
{
  // One wavefront per CTU, four horizontally adjacent CTUs per workgroup (their rows share 128-byte lines), sixteen samples per lane and
  // pass: luma in four passes of 16 rows (4 lanes across a row), U and V in one pass each (2 lanes across, 32 rows).  The parameter record
  // of a pass -- type, class, offsets -- is uniform over the wavefront, so no lane ever runs another CTU's branch.  Phase 1 only issues the
  // loads of all six passes (nothing in it consumes a loaded value), phase 2 computes and stores.
  const int lane = threadIdx.x & 63, cxi = blockIdx.x * 4 + (threadIdx.x >> 6), cyi = blockIdx.y, frame = blockIdx.z;
  const int wc = (W + 63) >> 6, hc = (H + 63) >> 6;
  if (cxi >= wc) return;
  const long frame_off = (long)frame * ((long)W * H * 3 / 2);
  // The records: packed by the SAO decision kernels of the batch (kvz_sao.hpp SaoRec), or built here from the caller's parameter structures
  const long ctu = (long)frame * wc * hc + (long)cyi * wc + cxi;
  unsigned long long rec3[3];
  for (int c = 0; c < 3; c++) {
    if (packed) rec3[c] = packed[ctu * 3 + c];
    else {
      const kvz_hip_sao_params *q = c ? &chroma[ctu] : &luma[ctu];
      const int base = c == 2 ? 5 : 0;
      unsigned long long v = (unsigned long long)(q->type & 0xff) | ((unsigned long long)(q->eo_class & 0xff) << 8) | ((unsigned long long)(q->band_position[c == 2 ? 1 : 0] & 0xff) << 16);
      for (int k = 0; k < 5; k++) v |= (unsigned long long)(u8)(int8_t)q->offsets[base + k] << (24 + 8 * k);
      rec3[c] = v;
    }
  }
  uint4 c16[6], a16[6], b16[6];
  long at[6];      // byte index of the pass's first sample, -1: outside the picture
  int geo[6];      // nvalid (dwords inside the picture) | (adj_a + 1) << 4 | (adj_b + 1) << 8 | first-sample-at-x0 << 12 | last-sample-at-row-end << 13 | row-at-picture-edge << 14
#pragma unroll
  for (int p = 0; p < 6; p++) {
    const int color = p < 4 ? 0 : p - 3, sh = color ? 1 : 0, fw = W >> sh, fh = H >> sh, bw = 64 >> sh;
    const long plane = frame_off + (color == 0 ? 0 : (color == 1 ? (long)W * H : (long)W * H * 5 / 4));
    const u32 rlo = (u32)rec3[color];
    const int type = (int)(rlo & 0xff), cls = (int)((rlo >> 8) & 0xff);
    const int x = cxi * bw + 16 * (color ? lane & 1 : lane & 3), y = cyi * bw + (color ? lane >> 1 : (lane >> 2) + 16 * p);
    at[p] = -1; geo[p] = 0;
    c16[p] = a16[p] = b16[p] = make_uint4(0, 0, 0, 0);
    if (x < fw && y < fh) {
      const u8 *row = in + plane + (long)y * fw;
      const int nvalid = (!TAIL || fw - x >= 16) ? 4 : (fw - x) >> 2;
      at[p] = plane + (long)y * fw + x;
      const int dx = cls == 1 ? 0 : (cls == 3 ? 1 : -1);           // a = (dx, -1 or 0), b = (-dx, +1 or 0)  (sao.h:71-76)
      // clamped rows: samples whose neighbour row is outside keep their value
      const int ra = (cls == 0 || y == 0) ? 0 : -fw, rb = (cls == 0 || y + 1 == fh) ? 0 : fw;
      // neighbour samples; at the ends of the row the load is moved inside the row and the bytes shifted into place in phase 2 (the byte
      // that falls off belongs to a sample that keeps its value)
      const int last = x + 4 * nvalid;  // one past the last valid sample of this lane
      const int adj_a = (x + dx < 0) ? 1 : ((last + dx > fw) ? -1 : 0), adj_b = (x - dx < 0) ? 1 : ((last - dx > fw) ? -1 : 0);
      geo[p] = nvalid | ((adj_a + 1) << 4) | ((adj_b + 1) << 8) | ((x == 0) << 12) | ((last == fw) << 13) | ((y == 0 || y + 1 == fh) << 14);
      const u8 *pa = row + ra + x + dx + adj_a, *pb = row + rb + x - dx + adj_b;
      if (!TAIL || nvalid == 4) {
        c16[p] = *reinterpret_cast<const uint4 *>(row + x);
        if (type == 2) { a16[p] = load_u128_any(pa); b16[p] = load_u128_any(pb); }
      } else {
        if (nvalid > 0) { c16[p].x = *reinterpret_cast<const u32 *>(row + x); if (type == 2) { a16[p].x = load_u32_any(pa); b16[p].x = load_u32_any(pb); } }
        if (nvalid > 1) { c16[p].y = *reinterpret_cast<const u32 *>(row + x + 4); if (type == 2) { a16[p].y = load_u32_any(pa + 4); b16[p].y = load_u32_any(pb + 4); } }
        if (nvalid > 2) { c16[p].z = *reinterpret_cast<const u32 *>(row + x + 8); if (type == 2) { a16[p].z = load_u32_any(pa + 8); b16[p].z = load_u32_any(pb + 8); } }
      }
    }
  }
#pragma unroll
  for (int p = 0; p < 6; p++) {
    const int color = p < 4 ? 0 : p - 3;
    const unsigned long long rec = rec3[color];
    const u32 rlo = (u32)rec, rhi = (u32)(rec >> 32);             // bytes: type, class, band position, offsets[0] | offsets[1..4]
    const int type = (int)(rlo & 0xff), cls = (int)((rlo >> 8) & 0xff);
    if (at[p] < 0) continue;
    const int nvalid = geo[p] & 15, adj_a = ((geo[p] >> 4) & 3) - 1, adj_b = ((geo[p] >> 8) & 3) - 1;
    u32 res[4];
    uint4 a = a16[p], b = b16[p];
    u32 keep_first = 0xffffffffu, keep_last = 0xffffffffu, whole = 0xffffffffu;
    if (type == 2) {
      if (adj_a > 0) a = shl8_u128(a); else if (adj_a < 0) a = shr8_u128(a);
      if (adj_b > 0) b = shl8_u128(b); else if (adj_b < 0) b = shr8_u128(b);
      // samples with a neighbour outside the picture keep their value (sao.c:324-349)
      if (cls != 0 && ((geo[p] >> 14) & 1)) whole = 0;
      if (cls != 1) { if ((geo[p] >> 12) & 1) keep_first = 0xffffff00u; if ((geo[p] >> 13) & 1) keep_last = 0x00ffffffu; }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const u32 c4 = i == 0 ? c16[p].x : (i == 1 ? c16[p].y : (i == 2 ? c16[p].z : c16[p].w));
      const u32 a4 = i == 0 ? a.x : (i == 1 ? a.y : (i == 2 ? a.z : a.w)), b4 = i == 0 ? b.x : (i == 1 ? b.y : (i == 2 ? b.z : b.w));
      res[i] = c4;
      if (type == 1) {
        const u32 bh = (1u - ((rlo >> 16) & 0xff)) & 0xffffu;
        const dev_pk16 bias = __builtin_bit_cast(dev_pk16, bh | (bh << 16));  // + 1 - band position in both halves
        const u32 band = (c4 >> 3) & 0x1f1f1f1fu;
        const dev_pk16 lo = { 0, 0 }, five = { 5, 5 };
        const dev_pk16 te = __builtin_elementwise_min(__builtin_elementwise_max(__builtin_bit_cast(dev_pk16, band & 0x00ff00ffu) + bias, lo), five);
        const dev_pk16 to = __builtin_elementwise_min(__builtin_elementwise_max(__builtin_bit_cast(dev_pk16, (band >> 8) & 0x00ff00ffu) + bias, lo), five);
        const u32 t4 = __builtin_bit_cast(u32, te) | (__builtin_bit_cast(u32, to) << 8);
        const u32 sel = __builtin_amdgcn_perm(0x00000c07u, 0x0605040cu, t4);  // 0 -> zero, 1..4 -> offsets[1..4], 5 -> zero
        res[i] = sao_add_offsets(c4, __builtin_amdgcn_perm(rhi, rlo, sel));
      } else if (type == 2) {
        const u32 idx4 = sao_sign_idx(c4, a4, b4);
        const u32 sel = __builtin_amdgcn_perm(0x00000007u, 0x06030504u, idx4);  // {1,2,0,3,4}[idx] as byte positions of the record
        u32 keep = whole;
        if (i == 0) keep &= keep_first;
        if (i == nvalid - 1) keep &= keep_last;
        res[i] = sao_add_offsets(c4, __builtin_amdgcn_perm(rhi, rlo, sel) & keep);
      }
    }
    if (!TAIL || nvalid == 4) *reinterpret_cast<uint4 *>(out + at[p]) = make_uint4(res[0], res[1], res[2], res[3]);
    else {
      if (nvalid > 0) *reinterpret_cast<u32 *>(out + at[p]) = res[0];
      if (nvalid > 1) *reinterpret_cast<u32 *>(out + at[p] + 4) = res[1];
      if (nvalid > 2) *reinterpret_cast<u32 *>(out + at[p] + 8) = res[2];
    }
  }
}
inline void launch_sao(hipStream_t stream, const u8 *in, u8 *out, int W, int H, int n_frames, const unsigned long long *packed, const kvz_hip_sao_params *luma, const kvz_hip_sao_params *chroma)
{
  const long fb = (long)W * H * 3 / 2, lcus = (long)((W + 63) >> 6) * ((H + 63) >> 6);
  for (int f0 = 0; f0 < n_frames; f0 += 32768) {  // gridDim.z <= 65535
    const int nf = n_frames - f0 < 32768 ? n_frames - f0 : 32768;
    const dim3 grid((unsigned)((((W + 63) >> 6) + 3) >> 2), (unsigned)((H + 63) >> 6), (unsigned)nf);
    const unsigned long long *pk = packed ? packed + 3 * lcus * f0 : nullptr;
    const kvz_hip_sao_params *lu = luma ? luma + lcus * f0 : nullptr, *ch = chroma ? chroma + lcus * f0 : nullptr;
    if ((W >> 1) % 16 == 0) hipLaunchKernelGGL(dev_sao_kernel<false>, grid, dim3(256), 0, stream, in + f0 * fb, out + f0 * fb, W, H, pk, lu, ch);
    else hipLaunchKernelGGL(dev_sao_kernel<true>, grid, dim3(256), 0, stream, in + f0 * fb, out + f0 * fb, W, H, pk, lu, ch);
  }
}

// beta / tc / tc_c / tc1: the thresholds of the launch's one QP.  qp_of_picture != nullptr (device, a QP per picture: kvz_hip_batch_loop_filters_models): every picture's
// own, derived where they are used from beta_off / tc_off
struct DeblockThresholds { int beta, tc, tc_c, tc1; };
struct DeblockGeom { int W, H, beta, tc, tc_c; long frame_bytes; const u8 *cu_depth; const kvz_hip_cu_dbk *info; int slice_b, tc1; /* inter pictures: per-4x4 records, tc at strength 1 */
                     const int32_t *qp_of_picture; int beta_off, tc_off; };
KVZ_HD DeblockThresholds deblock_thresholds(int qp, int beta_off, int tc_off)
{
  DeblockThresholds t;
  t.tc1 = deblock_tc(iclip(0, 53, qp + 2 * tc_off));  // filter.c:496-497 with strength 1
  t.beta = deblock_beta(iclip(0, 51, qp + 2 * beta_off));
  t.tc = deblock_tc(iclip(0, 53, qp + 2 + 2 * tc_off));                  // filter.c:496-497 with strength 2
  t.tc_c = deblock_tc(iclip(0, 53, chroma_qp(qp) + 2 + 2 * tc_off));  // filter.c:592-595
  return t;
}
__device__ __forceinline__ DeblockThresholds deblock_thresholds_of(const DeblockGeom &g, long frame)
{
  if (g.qp_of_picture) return deblock_thresholds(g.qp_of_picture[frame], g.beta_off, g.tc_off);
  const DeblockThresholds t = { g.beta, g.tc, g.tc_c, g.tc1 };
  return t;
}

__device__ __forceinline__ bool deblock_edge_on(const DeblockGeom &g, long frame, int x, int y, bool vertical)  // filter.c:202-216
{
  const int w8 = g.W >> 3, d = g.cu_depth[frame * (long)w8 * (g.H >> 3) + (long)(y >> 3) * w8 + (x >> 3)];
  const int tu_w = 64 >> (d ? d : 1);
  return ((vertical ? x : y) & (tu_w - 1)) == 0;
}
// Inter pictures: is the 8x8 unit at (ux, uy) on a transform or prediction edge (filter.c:202-257), and how strong is the 4-sample part whose first
// sample on the q side is (x, y) (filter.c:405-493)?  One record per 4x4 unit.
__device__ __forceinline__ const kvz_hip_cu_dbk *dbk_unit(const DeblockGeom &g, long frame, int x, int y)
{
  return g.info + frame * ((long)(g.W >> 2) * (g.H >> 2)) + (long)(y >> 2) * (g.W >> 2) + (x >> 2);
}
__device__ __forceinline__ bool dbk_edge_on_inter(const DeblockGeom &g, long frame, int ux, int uy, bool vertical)
{
  const kvz_hip_cu_dbk *u = dbk_unit(g, frame, ux, uy);
  const int pos = vertical ? ux : uy;
  if ((pos & ((64 >> u->tr_depth) - 1)) == 0) return true;  // transform edge
  const int cu_w = 64 >> u->depth, rel = pos & (cu_w - 1);  // prediction edges of the CU's partitioning, in quarters of the CU (cu.c:63-72)
  if (rel == 0) return true;
  const int ps = u->part_size;
  int q = -1;  // the second partition's offset along this axis, if it has one
  if (vertical) q = (ps == 2 || ps == 3) ? 2 : (ps == 6 ? 1 : (ps == 7 ? 3 : -1));
  else q = (ps == 1 || ps == 3) ? 2 : (ps == 4 ? 1 : (ps == 5 ? 3 : -1));
  return q >= 0 && rel == q * cu_w / 4;
}
__device__ __forceinline__ int dbk_strength(const DeblockGeom &g, long frame, int x, int y, bool vertical, bool tu_boundary)
{
  const kvz_hip_cu_dbk *q = dbk_unit(g, frame, x, y), *p = dbk_unit(g, frame, vertical ? x - 1 : x, vertical ? y : y - 1);
  if (q->type == 1 || p->type == 1) return 2;
  if (tu_boundary && (q->cbf_y || p->cbf_y)) return 1;
  auto far = [](int a, int b) { return iabs(a - b) >= 4; };
  if (p->mv_dir != 3 && q->mv_dir != 3) {
    const int lq = q->mv_dir - 1, lp = p->mv_dir - 1;
    if (far(q->mv[lq][0], p->mv[lp][0]) || far(q->mv[lq][1], p->mv[lp][1])) return 1;
    if (q->mv_ref[lq] != p->mv_ref[lp]) return 1;
  }
  if (!g.slice_b) return 0;
  // B slices (filter.c:428-489): undefined vectors count as zero, references compared as pictures
  const int rp0 = (p->mv_dir & 1) ? p->ref_id[0] : -1, rp1 = (p->mv_dir & 2) ? p->ref_id[1] : -1;
  const int rq0 = (q->mv_dir & 1) ? q->ref_id[0] : -1, rq1 = (q->mv_dir & 2) ? q->ref_id[1] : -1;
  const int q0x = (q->mv_dir & 1) ? q->mv[0][0] : 0, q0y = (q->mv_dir & 1) ? q->mv[0][1] : 0, q1x = (q->mv_dir & 2) ? q->mv[1][0] : 0, q1y = (q->mv_dir & 2) ? q->mv[1][1] : 0;
  const int p0x = (p->mv_dir & 1) ? p->mv[0][0] : 0, p0y = (p->mv_dir & 1) ? p->mv[0][1] : 0, p1x = (p->mv_dir & 2) ? p->mv[1][0] : 0, p1y = (p->mv_dir & 2) ? p->mv[1][1] : 0;
  if (!((rp0 == rq0 && rp1 == rq1) || (rp0 == rq1 && rp1 == rq0))) return 1;
  const bool straight = far(q0x, p0x) || far(q0y, p0y) || far(q1x, p1x) || far(q1y, p1y);
  const bool crossed = far(q1x, p0x) || far(q1y, p0y) || far(q0x, p1x) || far(q0y, p1y);
  if (rp0 != rp1) return (rp0 == rq0 ? straight : crossed) ? 1 : 0;
  return (straight && crossed) ? 1 : 0;
}
// Luma filter of one 4-line part (filter.c:386-561): sample k of a line, the edge between k = 3 and k = 4.
// Two lines per operation: P[p][k] = sample k of lines 2 p (low half) and 2 p + 1 (high half) as int16.  Every intermediate fits
// 16 bits (|9 (m4 - m3) - 3 (m5 - m2) + 8| <= 3068, sums of up to 8 samples + 4 <= 2044); per-line conditions become 0 / -1 half masks.
__device__ __forceinline__ dev_pk16 pk_splat(int v) { const dev_pk16 r = { (short)v, (short)v }; return r; }
__device__ __forceinline__ dev_pk16 pk_abs(dev_pk16 a) { return __builtin_elementwise_max(a, -a); }
__device__ __forceinline__ dev_pk16 pk_clip(dev_pk16 lo, dev_pk16 hi, dev_pk16 v) { return __builtin_elementwise_min(__builtin_elementwise_max(v, lo), hi); }
__device__ __forceinline__ dev_pk16 pk_select(dev_pk16 mask, dev_pk16 a, dev_pk16 b)  // mask halves 0 / -1: a where set, else b
{
  const u32 m = __builtin_bit_cast(u32, mask);
  return __builtin_bit_cast(dev_pk16, (__builtin_bit_cast(u32, a) & m) | (__builtin_bit_cast(u32, b) & ~m));
}
__device__ __forceinline__ void deblock_luma_lines_pk(dev_pk16 P[2][8], int beta, int tc)
{
  // decisions on lines 0 and 3 (filter.c:386-561): second differences of every line, then the two that count
  const dev_pk16 dpA = pk_abs(P[0][1] - P[0][2] - P[0][2] + P[0][3]), dqA = pk_abs(P[0][4] - P[0][5] - P[0][5] + P[0][6]);
  const dev_pk16 dpB = pk_abs(P[1][1] - P[1][2] - P[1][2] + P[1][3]), dqB = pk_abs(P[1][4] - P[1][5] - P[1][5] + P[1][6]);
  const int dp0 = dpA.x, dq0 = dqA.x, dp3 = dpB.y, dq3 = dqB.y;
  const int dp = dp0 + dp3, dq = dq0 + dq3;
  if (dp + dq >= beta) return;
  const int p00 = P[0][0].x, p03 = P[0][3].x, p04 = P[0][4].x, p07 = P[0][7].x, p30 = P[1][0].y, p33 = P[1][3].y, p34 = P[1][4].y, p37 = P[1][7].y;
  const bool strong = 2 * (dp0 + dq0) < (beta >> 2) && 2 * (dp3 + dq3) < (beta >> 2) &&
                      iabs(p03 - p04) < ((5 * tc + 1) >> 1) && iabs(p33 - p34) < ((5 * tc + 1) >> 1) &&
                      iabs(p00 - p03) + iabs(p04 - p07) < (beta >> 3) && iabs(p30 - p33) + iabs(p34 - p37) < (beta >> 3);
  const int side = (beta + (beta >> 1)) >> 3;
  const dev_pk16 zero = pk_splat(0), maxv = pk_splat(255);
#pragma unroll
  for (int p = 0; p < 2; p++) {
    const dev_pk16 m0 = P[p][0], m1 = P[p][1], m2 = P[p][2], m3 = P[p][3], m4 = P[p][4], m5 = P[p][5], m6 = P[p][6], m7 = P[p][7];
    if (strong) {
      const dev_pk16 t2 = pk_splat(2 * tc), c2 = pk_splat(2), c4 = pk_splat(4);
      const dev_pk16 s34 = m3 + m4;
      P[p][1] = pk_clip(m1 - t2, m1 + t2, (m0 + m0 + m1 + m1 + m1 + m2 + s34 + c4) >> 3);
      P[p][2] = pk_clip(m2 - t2, m2 + t2, (m1 + m2 + s34 + c2) >> 2);
      P[p][3] = pk_clip(m3 - t2, m3 + t2, (m1 + m2 + m2 + s34 + s34 + m5 + c4) >> 3);
      P[p][4] = pk_clip(m4 - t2, m4 + t2, (m2 + s34 + s34 + m5 + m5 + m6 + c4) >> 3);
      P[p][5] = pk_clip(m5 - t2, m5 + t2, (s34 + m5 + m6 + c2) >> 2);
      P[p][6] = pk_clip(m6 - t2, m6 + t2, (s34 + m5 + m6 + m6 + m6 + m7 + m7 + c4) >> 3);
    } else {
      const dev_pk16 d43 = m4 - m3, d52 = m5 - m2;
      dev_pk16 delta = ((d43 << 3) + d43 - d52 - d52 - d52 + pk_splat(8)) >> 4;
      const dev_pk16 on = (pk_abs(delta) - pk_splat(tc * 10)) >> 15;  // -1 where |delta| < 10 tc
      const dev_pk16 tcv = pk_splat(tc), tc2 = pk_splat(tc >> 1), one = pk_splat(1);
      delta = pk_clip(-tcv, tcv, delta);
      P[p][3] = pk_select(on, pk_clip(zero, maxv, m3 + delta), m3);
      P[p][4] = pk_select(on, pk_clip(zero, maxv, m4 - delta), m4);
      if (dp < side) P[p][2] = pk_select(on, pk_clip(zero, maxv, m2 + pk_clip(-tc2, tc2, ((((m1 + m3 + one) >> 1) - m2 + delta) >> 1))), m2);
      if (dq < side) P[p][5] = pk_select(on, pk_clip(zero, maxv, m5 + pk_clip(-tc2, tc2, ((((m6 + m4 + one) >> 1) - m5 - delta) >> 1))), m5);
    }
  }
}
// Luma.  VERTICAL: part (x = 8 * x8, y = 4 * y4): 4 rows of the 8 samples x - 4 .. x + 3 (one 8-byte access per row, 4-byte
// aligned); !VERTICAL: part (x = 4 * x4, y = 8 * y8): the 8 rows y - 4 .. y + 3 of 4 samples (one dword per row).
// CUQP (kvz_hip_batch_loop_filters_ctu_models): cu_qp is the plane of CU QPs of the pictures (kvz_cu_qp.hpp), a byte per 8x8 unit, and an edge part is filtered at
// (QpP + QpQ + 1) >> 1 of the units on its two sides (filter.c:275-295 get_qp_y_pred; (x, y): the part's first luma sample on the q side)
__device__ __forceinline__ int deblock_edge_qp(const DeblockGeom &g, const u8 *cu_qp, long frame, int x, int y, bool vertical)
{
  const int w8 = g.W >> 3;
  const u8 *plane = cu_qp + frame * (long)w8 * (g.H >> 3);
  const int qp_q = plane[(long)(y >> 3) * w8 + (x >> 3)], qp_p = vertical ? plane[(long)(y >> 3) * w8 + ((x - 1) >> 3)] : plane[(long)((y - 1) >> 3) * w8 + (x >> 3)];
  return (qp_p + qp_q + 1) >> 1;
}
template <bool VERTICAL> __global__ void __launch_bounds__(256) dev_deblock_luma_kernel(u8 *frames, const DeblockGeom g, const long parts)
{
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= parts) return;
  const int nx = VERTICAL ? g.W >> 3 : g.W >> 2, ny = VERTICAL ? g.H >> 2 : g.H >> 3;
  const long frame = p / ((long)nx * ny);
  const int r = (int)(p % ((long)nx * ny)), ix = r % nx, iy = r / nx;
  const int x = VERTICAL ? 8 * ix : 4 * ix, y = VERTICAL ? 4 * iy : 8 * iy;
  if ((VERTICAL ? x : y) == 0) return;
  const DeblockThresholds thr = deblock_thresholds_of(g, frame);
  int tc = thr.tc;
  if (g.info) {  // inter picture: edge test on the 8x8 unit, strength per 4-sample part
    const int ux = x & ~7, uy = y & ~7;
    if (!dbk_edge_on_inter(g, frame, ux, uy, VERTICAL)) return;
    const kvz_hip_cu_dbk *u = dbk_unit(g, frame, ux, uy);
    const int strength = dbk_strength(g, frame, x, y, VERTICAL, (((VERTICAL ? ux : uy)) & ((64 >> u->tr_depth) - 1)) == 0);
    if (!strength) return;
    if (strength == 1) tc = thr.tc1;
  } else if (!deblock_edge_on(g, frame, x, y, VERTICAL)) return;
  u8 *Y = frames + frame * g.frame_bytes;
  dev_pk16 P[2][8];
  if (VERTICAL) {
    u32 lo[4], hi[4];
    for (int i = 0; i < 4; i++) {
      const u32 *row = reinterpret_cast<const u32 *>(Y + (long)(y + i) * g.W + x - 4);
      lo[i] = row[0]; hi[i] = row[1];
    }
    for (int p = 0; p < 2; p++)
      for (int k = 0; k < 4; k++) {  // byte k of line 2 p -> low half, of line 2 p + 1 -> high half
        const u32 sel = 0x0c000c00u | (u32)k | ((u32)(4 + k) << 16);
        P[p][k] = __builtin_bit_cast(dev_pk16, __builtin_amdgcn_perm(lo[2 * p + 1], lo[2 * p], sel));
        P[p][4 + k] = __builtin_bit_cast(dev_pk16, __builtin_amdgcn_perm(hi[2 * p + 1], hi[2 * p], sel));
      }
  } else {
    for (int k = 0; k < 8; k++) {
      const u32 v = *reinterpret_cast<const u32 *>(Y + (long)(y - 4 + k) * g.W + x);
      P[0][k] = __builtin_bit_cast(dev_pk16, __builtin_amdgcn_perm(v, v, 0x0c010c00u));
      P[1][k] = __builtin_bit_cast(dev_pk16, __builtin_amdgcn_perm(v, v, 0x0c030c02u));
    }
  }
  deblock_luma_lines_pk(P, thr.beta, tc);
  if (VERTICAL) {
    for (int p = 0; p < 2; p++) {
      // halves (k0 | k1 << 8) and (k2 | k3 << 8) of both lines, then one dword per line
      const u32 a01 = __builtin_bit_cast(u32, P[p][0]) | (__builtin_bit_cast(u32, P[p][1]) << 8), a23 = __builtin_bit_cast(u32, P[p][2]) | (__builtin_bit_cast(u32, P[p][3]) << 8);
      const u32 a45 = __builtin_bit_cast(u32, P[p][4]) | (__builtin_bit_cast(u32, P[p][5]) << 8), a67 = __builtin_bit_cast(u32, P[p][6]) | (__builtin_bit_cast(u32, P[p][7]) << 8);
      u32 *r0 = reinterpret_cast<u32 *>(Y + (long)(y + 2 * p) * g.W + x - 4), *r1 = reinterpret_cast<u32 *>(Y + (long)(y + 2 * p + 1) * g.W + x - 4);
      r0[0] = __builtin_amdgcn_perm(a23, a01, 0x05040100u); r0[1] = __builtin_amdgcn_perm(a67, a45, 0x05040100u);
      r1[0] = __builtin_amdgcn_perm(a23, a01, 0x07060302u); r1[1] = __builtin_amdgcn_perm(a67, a45, 0x07060302u);
    }
  } else {
    for (int k = 1; k < 7; k++)
      *reinterpret_cast<u32 *>(Y + (long)(y - 4 + k) * g.W + x) = __builtin_amdgcn_perm(__builtin_bit_cast(u32, P[1][k]), __builtin_bit_cast(u32, P[0][k]), 0x06040200u);
  }
}
// ... of all-intra pictures with a QP per CU: the kernel above with the thresholds of the part's own edge QP, taken behind the edge test.  A kernel of its own with a
// body of its own -- moving the body above into a function that both instantiate made the compiler schedule the existing kernels differently, and those stay what they were.
template <bool VERTICAL> __global__ void __launch_bounds__(256) dev_deblock_luma_kernel_cuqp(u8 *frames, const DeblockGeom g, const long parts, const u8 *cu_qp)
{
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= parts) return;
  const int nx = VERTICAL ? g.W >> 3 : g.W >> 2, ny = VERTICAL ? g.H >> 2 : g.H >> 3;
  const long frame = p / ((long)nx * ny);
  const int r = (int)(p % ((long)nx * ny)), ix = r % nx, iy = r / nx;
  const int x = VERTICAL ? 8 * ix : 4 * ix, y = VERTICAL ? 4 * iy : 8 * iy;
  if ((VERTICAL ? x : y) == 0) return;
  if (!deblock_edge_on(g, frame, x, y, VERTICAL)) return;
  const DeblockThresholds thr = deblock_thresholds(deblock_edge_qp(g, cu_qp, frame, x, y, VERTICAL), g.beta_off, g.tc_off);
  u8 *Y = frames + frame * g.frame_bytes;
  dev_pk16 P[2][8];
  if (VERTICAL) {
    u32 lo[4], hi[4];
    for (int i = 0; i < 4; i++) {
      const u32 *row = reinterpret_cast<const u32 *>(Y + (long)(y + i) * g.W + x - 4);
      lo[i] = row[0]; hi[i] = row[1];
    }
    for (int p = 0; p < 2; p++)
      for (int k = 0; k < 4; k++) {  // byte k of line 2 p -> low half, of line 2 p + 1 -> high half
        const u32 sel = 0x0c000c00u | (u32)k | ((u32)(4 + k) << 16);
        P[p][k] = __builtin_bit_cast(dev_pk16, __builtin_amdgcn_perm(lo[2 * p + 1], lo[2 * p], sel));
        P[p][4 + k] = __builtin_bit_cast(dev_pk16, __builtin_amdgcn_perm(hi[2 * p + 1], hi[2 * p], sel));
      }
  } else {
    for (int k = 0; k < 8; k++) {
      const u32 v = *reinterpret_cast<const u32 *>(Y + (long)(y - 4 + k) * g.W + x);
      P[0][k] = __builtin_bit_cast(dev_pk16, __builtin_amdgcn_perm(v, v, 0x0c010c00u));
      P[1][k] = __builtin_bit_cast(dev_pk16, __builtin_amdgcn_perm(v, v, 0x0c030c02u));
    }
  }
  deblock_luma_lines_pk(P, thr.beta, thr.tc);
  if (VERTICAL) {
    for (int p = 0; p < 2; p++) {
      const u32 a01 = __builtin_bit_cast(u32, P[p][0]) | (__builtin_bit_cast(u32, P[p][1]) << 8), a23 = __builtin_bit_cast(u32, P[p][2]) | (__builtin_bit_cast(u32, P[p][3]) << 8);
      const u32 a45 = __builtin_bit_cast(u32, P[p][4]) | (__builtin_bit_cast(u32, P[p][5]) << 8), a67 = __builtin_bit_cast(u32, P[p][6]) | (__builtin_bit_cast(u32, P[p][7]) << 8);
      u32 *r0 = reinterpret_cast<u32 *>(Y + (long)(y + 2 * p) * g.W + x - 4), *r1 = reinterpret_cast<u32 *>(Y + (long)(y + 2 * p + 1) * g.W + x - 4);
      r0[0] = __builtin_amdgcn_perm(a23, a01, 0x05040100u); r0[1] = __builtin_amdgcn_perm(a67, a45, 0x05040100u);
      r1[0] = __builtin_amdgcn_perm(a23, a01, 0x07060302u); r1[1] = __builtin_amdgcn_perm(a67, a45, 0x07060302u);
    }
  } else {
    for (int k = 1; k < 7; k++)
      *reinterpret_cast<u32 *>(Y + (long)(y - 4 + k) * g.W + x) = __builtin_amdgcn_perm(__builtin_bit_cast(u32, P[1][k]), __builtin_bit_cast(u32, P[0][k]), 0x06040200u);
  }
}
// Chroma (filter.c:567-632, 170-190): edges on the 8x8 chroma grid, 4 samples per part, both planes (part index carries the plane)
template <bool VERTICAL> __global__ void __launch_bounds__(256) dev_deblock_chroma_kernel(u8 *frames, const DeblockGeom g, const long parts)
{
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= parts) return;
  const int cw = g.W >> 1, ch = g.H >> 1;
  const int nx = VERTICAL ? (cw + 7) >> 3 : cw >> 2, ny = VERTICAL ? ch >> 2 : (ch + 7) >> 3;  // same counts as deblock_frames_on
  const long per_frame = 2L * nx * ny, frame = p / per_frame;
  const int r = (int)(p % per_frame), plane = r / (nx * ny), q = r % (nx * ny), ix = q % nx, iy = q / nx;
  const int xc = VERTICAL ? 8 * ix : 4 * ix, yc = VERTICAL ? 4 * iy : 8 * iy;
  if ((VERTICAL ? xc : yc) == 0) return;
  if (g.info) {  // filter.c:567-632: the unit's edge test, then only next to an intra CU (strength 2)
    if (!dbk_edge_on_inter(g, frame, 2 * xc, 2 * yc, VERTICAL)) return;
    const kvz_hip_cu_dbk *q = dbk_unit(g, frame, 2 * xc, 2 * yc), *pp = dbk_unit(g, frame, VERTICAL ? 2 * xc - 2 : 2 * xc, VERTICAL ? 2 * yc : 2 * yc - 2);
    if (q->type != 1 && pp->type != 1) return;
  } else if (!deblock_edge_on(g, frame, 2 * xc, 2 * yc, VERTICAL)) return;
  u8 *P = frames + frame * g.frame_bytes + (long)g.W * g.H + (long)plane * cw * ch;
  const int across = VERTICAL ? 1 : cw, along = VERTICAL ? cw : 1, tc_c = deblock_thresholds_of(g, frame).tc_c;
  for (int i = 0; i < 4; i++) {
    u8 *s = P + (long)yc * cw + xc + i * along;
    const int m2 = s[-2 * across], m3 = s[-across], m4 = s[0], m5 = s[across];
    const int delta = iclip(-tc_c, tc_c, (((m4 - m3) * 4) + m2 - m5 + 4) >> 3);
    s[-across] = (u8)iclip(0, 255, m3 + delta);
    s[0] = (u8)iclip(0, 255, m4 - delta);
  }
}
// ... of all-intra pictures with a QP per CU (a kernel of its own, as for luma): the chroma tc of the edge's luma QP through the chroma table (filter.c:588-592)
template <bool VERTICAL> __global__ void __launch_bounds__(256) dev_deblock_chroma_kernel_cuqp(u8 *frames, const DeblockGeom g, const long parts, const u8 *cu_qp)
{
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= parts) return;
  const int cw = g.W >> 1, ch = g.H >> 1;
  const int nx = VERTICAL ? (cw + 7) >> 3 : cw >> 2, ny = VERTICAL ? ch >> 2 : (ch + 7) >> 3;  // same counts as deblock_frames_on
  const long per_frame = 2L * nx * ny, frame = p / per_frame;
  const int r = (int)(p % per_frame), plane = r / (nx * ny), q = r % (nx * ny), ix = q % nx, iy = q / nx;
  const int xc = VERTICAL ? 8 * ix : 4 * ix, yc = VERTICAL ? 4 * iy : 8 * iy;
  if ((VERTICAL ? xc : yc) == 0) return;
  if (!deblock_edge_on(g, frame, 2 * xc, 2 * yc, VERTICAL)) return;
  u8 *P = frames + frame * g.frame_bytes + (long)g.W * g.H + (long)plane * cw * ch;
  const int across = VERTICAL ? 1 : cw, along = VERTICAL ? cw : 1;
  const int tc_c = deblock_thresholds(deblock_edge_qp(g, cu_qp, frame, 2 * xc, 2 * yc, VERTICAL), g.beta_off, g.tc_off).tc_c;
  for (int i = 0; i < 4; i++) {
    u8 *s = P + (long)yc * cw + xc + i * along;
    const int m2 = s[-2 * across], m3 = s[-across], m4 = s[0], m5 = s[across];
    const int delta = iclip(-tc_c, tc_c, (((m4 - m3) * 4) + m2 - m5 + 4) >> 3);
    s[-across] = (u8)iclip(0, 255, m3 + delta);
    s[0] = (u8)iclip(0, 255, m4 - delta);
  }
}

// passes: 1 = the vertical edges, 2 = the horizontal edges, 3 = both (in that order)
inline void deblock_frames_on(hipStream_t stream, u8 *frames, int width, int height, int n_frames, const u8 *cu_depth, int qp, int beta_off, int tc_off, int passes = 3,
                              const kvz_hip_cu_dbk *info = nullptr, int slice_b = 0, const int32_t *qp_of_picture = nullptr /* device: a QP per picture instead of `qp` */,
                              const u8 *cu_qp = nullptr /* device: a QP per 8x8 unit instead of either (all-intra pictures: the CUQP kernels) */)
{
  if (n_frames <= 0) return;
  DeblockGeom g;
  g.W = width; g.H = height; g.cu_depth = cu_depth; g.frame_bytes = (long)width * height * 3 / 2;
  g.info = info; g.slice_b = slice_b;
  const DeblockThresholds t = deblock_thresholds(qp, beta_off, tc_off);
  g.tc1 = t.tc1; g.beta = t.beta; g.tc = t.tc; g.tc_c = t.tc_c;
  g.qp_of_picture = qp_of_picture; g.beta_off = beta_off; g.tc_off = tc_off;
  const int cw = width >> 1, ch = height >> 1;
  auto grid = [](long n) { return dim3((unsigned)((n + 255) / 256)); };
  const long lv = (long)n_frames * (width >> 3) * (height >> 2), lh = (long)n_frames * (width >> 2) * (height >> 3);
  const long cv = 2L * n_frames * ((cw + 7) >> 3) * (ch >> 2), chh = 2L * n_frames * (cw >> 2) * ((ch + 7) >> 3);
  if (cu_qp) {
    if (lv && (passes & 1)) hipLaunchKernelGGL(dev_deblock_luma_kernel_cuqp<true>, grid(lv), dim3(256), 0, stream, frames, g, lv, cu_qp);
    if (cv && (passes & 1)) hipLaunchKernelGGL(dev_deblock_chroma_kernel_cuqp<true>, grid(cv), dim3(256), 0, stream, frames, g, cv, cu_qp);
    if (lh && (passes & 2)) hipLaunchKernelGGL(dev_deblock_luma_kernel_cuqp<false>, grid(lh), dim3(256), 0, stream, frames, g, lh, cu_qp);
    if (chh && (passes & 2)) hipLaunchKernelGGL(dev_deblock_chroma_kernel_cuqp<false>, grid(chh), dim3(256), 0, stream, frames, g, chh, cu_qp);
    KVZ_HIP_CHECK(hipGetLastError());
    return;
  }
  if (lv && (passes & 1)) hipLaunchKernelGGL(dev_deblock_luma_kernel<true>, grid(lv), dim3(256), 0, stream, frames, g, lv);
  if (cv && (passes & 1)) hipLaunchKernelGGL(dev_deblock_chroma_kernel<true>, grid(cv), dim3(256), 0, stream, frames, g, cv);
  if (lh && (passes & 2)) hipLaunchKernelGGL(dev_deblock_luma_kernel<false>, grid(lh), dim3(256), 0, stream, frames, g, lh);
  if (chh && (passes & 2)) hipLaunchKernelGGL(dev_deblock_chroma_kernel<false>, grid(chh), dim3(256), 0, stream, frames, g, chh);
  KVZ_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------------------------
// The "checksum" picture hash (nal-generic.c:57-82 array_checksum) of a batch: per plane the 32-bit wrap-around sum of sample ^ mask(x, y),
// mask = (x & 0xff) ^ (y & 0xff) ^ (x >> 8) ^ (y >> 8).  One workgroup per (plane, group of rows): a lane takes 16 samples of a row per step -- inside an
// aligned group of 16 the mask is one byte xor the position in the group, so four v_sad_u8 against 0 sum them -- and walks down the group's rows; the
// workgroup's sum goes out with one atomic add.  No divisions by run-time values (the first version spent its time in 64-bit index arithmetic: 160 GB/s).
__global__ void __launch_bounds__(256) dev_checksum_kernel(const u8 *frames, const int W, const int H, const long frame_bytes, const int rows_per_wg, u32 *out)
{
  __shared__ u32 s_sum[4];
  const int fp = blockIdx.y, frame = fp / 3, plane = fp - 3 * frame;
  const int pw = plane ? W >> 1 : W, ph = plane ? H >> 1 : H;
  const u8 *base = frames + frame * frame_bytes + (plane == 0 ? 0 : (plane == 1 ? (long)W * H : (long)W * H * 5 / 4));
  const int y0 = blockIdx.x * rows_per_wg, y1 = y0 + rows_per_wg < ph ? y0 + rows_per_wg : ph;
  u32 v = 0;
  if (y0 < ph) {
    if ((pw & 15) == 0) {
      const int units = pw >> 4;  // 16-sample units per row
      for (int i = threadIdx.x; i < units * (y1 - y0); i += 256) {
        const int ry = i / units, u = i - ry * units, y = y0 + ry, x = 16 * u;
        const uint4 w4 = *reinterpret_cast<const uint4 *>(base + (long)y * pw + x);
        const u32 c = (((x & 0xff) ^ (y & 0xff) ^ (x >> 8) ^ (y >> 8)) & 0xff) * 0x01010101u;
        v = __builtin_amdgcn_sad_u8(w4.x ^ c ^ 0x03020100u, 0u, v);
        v = __builtin_amdgcn_sad_u8(w4.y ^ c ^ 0x07060504u, 0u, v);
        v = __builtin_amdgcn_sad_u8(w4.z ^ c ^ 0x0b0a0908u, 0u, v);
        v = __builtin_amdgcn_sad_u8(w4.w ^ c ^ 0x0f0e0d0cu, 0u, v);
      }
    } else {  // widths that are multiples of 4 only: dword by dword
      const int units = pw >> 2;
      for (int i = threadIdx.x; i < units * (y1 - y0); i += 256) {
        const int ry = i / units, u = i - ry * units, y = y0 + ry, x = 4 * u;
        const u32 w = *reinterpret_cast<const u32 *>(base + (long)y * pw + x);
        const u32 c = (((x & 0xff) ^ (y & 0xff) ^ (x >> 8) ^ (y >> 8)) & 0xff) * 0x01010101u;
        v = __builtin_amdgcn_sad_u8(w ^ c ^ 0x03020100u, 0u, v);
      }
    }
  }
  v = group_sum<64>(v);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0 && y0 < ph) atomicAdd(&out[fp], s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]);
}
inline void launch_checksums(hipStream_t stream, const u8 *frames, int W, int H, int n_frames, u32 *out)
{
  const int rows = 32;  // 60 KB of a 1080p luma plane per workgroup
  const long fb = (long)W * H * 3 / 2;
  for (int f0 = 0; f0 < n_frames; f0 += 16384) {  // gridDim.y <= 65535
    const int nf = n_frames - f0 < 16384 ? n_frames - f0 : 16384;
    hipLaunchKernelGGL(dev_checksum_kernel, dim3((unsigned)((H + rows - 1) / rows), (unsigned)(3 * nf)), dim3(256), 0, stream, frames + (long)f0 * fb, W, H, fb, rows, out + 3L * f0);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Distortion of a batch (encmain.c:117-145 compute_psnr's sums): per (picture, plane) the exact sum of squared differences of two picture sets, 64 bits each.
// A plane is one run of bytes in both sets, a multiple of 16 long and 16-byte aligned, so this is a streaming reduction: a workgroup takes one piece of
// `units_per_piece` 16-byte units of a luma plane (a quarter of that of a chroma plane: every workgroup of the grid has work), a lane reads one unit of both sets
// per step, four steps' loads issued before the first use.  No byte is unpacked: sum (a - b)^2 = sum a a + sum b b - 2 sum a b, three v_dot4_u32_u8 per dword
// pair.  Range: a lane sees at most SSE_MAX_UNITS / 256 = 16 units, 64 dot products per accumulator, 64 * 260 100 < 2^25, and the workgroup's sum of squared
// differences is at most SSE_MAX_UNITS * 16 * 65 025 = 4 261 478 400 < 2^32 -- the wavefronts' sums are 32-bit, the workgroup's and the plane's 64-bit (a
// 3840x2160 plane of 0 against 255 is 5.4e11).  Integer adds only: the result does not depend on the schedule.
constexpr int SSE_MAX_UNITS = 4096;  // 64 KB of each set per workgroup
__device__ __forceinline__ void sse_unit(const uint4 x, const uint4 y, u32 &aa, u32 &bb, u32 &ab)
{
  aa = __builtin_amdgcn_udot4(x.x, x.x, aa, false); bb = __builtin_amdgcn_udot4(y.x, y.x, bb, false); ab = __builtin_amdgcn_udot4(x.x, y.x, ab, false);
  aa = __builtin_amdgcn_udot4(x.y, x.y, aa, false); bb = __builtin_amdgcn_udot4(y.y, y.y, bb, false); ab = __builtin_amdgcn_udot4(x.y, y.y, ab, false);
  aa = __builtin_amdgcn_udot4(x.z, x.z, aa, false); bb = __builtin_amdgcn_udot4(y.z, y.z, bb, false); ab = __builtin_amdgcn_udot4(x.z, y.z, ab, false);
  aa = __builtin_amdgcn_udot4(x.w, x.w, aa, false); bb = __builtin_amdgcn_udot4(y.w, y.w, bb, false); ab = __builtin_amdgcn_udot4(x.w, y.w, ab, false);
}
__global__ void __launch_bounds__(256) dev_sse_kernel(const u8 *a, const u8 *b, const int W, const int H, const long frame_bytes, const int units_per_piece, unsigned long long *out)
{
  __shared__ u32 s_sum[4];
  const int fp = blockIdx.y, frame = fp / 3, plane = fp - 3 * frame;
  const long luma = (long)W * H, offset = frame * frame_bytes + (plane == 0 ? 0 : (plane == 1 ? luma : luma * 5 / 4));
  const int units = (int)((plane ? luma >> 2 : luma) >> 4), per = plane ? units_per_piece >> 2 : units_per_piece;  // (a 16 320 x 16 320 plane is 16.6 M units)
  const uint4 *pa = reinterpret_cast<const uint4 *>(a + offset), *pb = reinterpret_cast<const uint4 *>(b + offset);
  const int begin = blockIdx.x * per, end = begin + per < units ? begin + per : units;
  u32 aa = 0, bb = 0, ab = 0;
  int i = begin + threadIdx.x;
  for (; i + 768 < end; i += 1024) {
    const uint4 x0 = pa[i], x1 = pa[i + 256], x2 = pa[i + 512], x3 = pa[i + 768];
    const uint4 y0 = pb[i], y1 = pb[i + 256], y2 = pb[i + 512], y3 = pb[i + 768];
    sse_unit(x0, y0, aa, bb, ab); sse_unit(x1, y1, aa, bb, ab); sse_unit(x2, y2, aa, bb, ab); sse_unit(x3, y3, aa, bb, ab);
  }
  for (; i < end; i += 256) sse_unit(pa[i], pb[i], aa, bb, ab);
  const u32 v = group_sum<64>(aa + bb - 2 * ab);  // exact in 32 bits: the lane's own sum of squares, see above
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0 && begin < units) atomicAdd(&out[fp], (unsigned long long)s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]);
}
__global__ void __launch_bounds__(256) dev_copy_u64_kernel(const unsigned long long *src, unsigned long long *dst, const int n)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}
// out [n_frames x 3] must be zero when the first launch starts (the callers queue a hipMemsetAsync in front)
inline void launch_sse(hipStream_t stream, const u8 *a, const u8 *b, int W, int H, int n_frames, unsigned long long *out)
{
  const long fb = (long)W * H * 3 / 2, luma_units = (long)W * H / 16;
  // pieces of 64 KB; of 16 KB at least (one step of four loads per lane) while the grid is smaller than a few workgroups per CU: one picture fills the device too
  int per = SSE_MAX_UNITS;
  while (per > 1024 && 3L * n_frames * ((luma_units + per - 1) / per) < 2048) per >>= 1;
  const unsigned pieces = (unsigned)((luma_units + per - 1) / per);
  for (int f0 = 0; f0 < n_frames; f0 += 16384) {  // gridDim.y <= 65535
    const int nf = n_frames - f0 < 16384 ? n_frames - f0 : 16384;
    hipLaunchKernelGGL(dev_sse_kernel, dim3(pieces, (unsigned)(3 * nf)), dim3(256), 0, stream, a + (long)f0 * fb, b + (long)f0 * fb, W, H, fb, per, out + 3L * f0);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// SAO parameter decision (kvz_sao.hpp): statistics + context-free candidates, one workgroup per (LCU, plane) ...
struct SaoGeom { int W, H, wl, hl; long frame_bytes; };
__global__ void __launch_bounds__(256) dev_sao_stats_kernel(const u8 *src, const u8 *R, const u8 *V, const u8 *D, const SaoGeom g, SaoStats *stats, SaoCand *cand)
{
  // accumulators: {sum, count} of a statistic packed into one 64-bit LDS word (sum in the high half, count in the low half: one ds_add_u64 per
  // sample and statistic; the count never carries into the sum -- at most 4096 samples).  Category 0 of the edge classes is never read by the
  // decision (its offset is 0 by definition, sao.c:417-418), so samples of category 0 -- the majority -- touch the band histogram only.
  // Sixteen private copies of the 52 accumulators, interleaved so that copy c lives in LDS banks 2 c, 2 c + 1: the lanes of a wavefront that hit the same
  // statistic no longer serialise on one address (one atomic per cycle and CU was the whole kernel: 34 ms per 1 536 pictures).
  constexpr int NACC = 4 * 5 + 32, COPIES = 16;
  __shared__ unsigned long long acc[NACC * COPIES];
  __shared__ SaoStats st;
  __shared__ u8 s_rec[64 * 64], s_org[64 * 64];
  const long item = blockIdx.x;  // (frame, lcu, plane)
  const int color = (int)(item % 3);
  const long lcu_all = item / 3;
  const int lcus = g.wl * g.hl, lcu = (int)(lcu_all % lcus);
  const long frame = lcu_all / lcus;
  const int lx = lcu % g.wl, ly = lcu / g.wl, sh = color ? 1 : 0, n = 64 >> sh, fw = g.W >> sh, fh = g.H >> sh;
  const long plane = frame * g.frame_bytes + (color == 0 ? 0 : (color == 1 ? (long)g.W * g.H : (long)g.W * g.H * 5 / 4));
  const int bw = imin(n, fw - lx * n), bh = imin(n, fh - ly * n);  // sao.c:598-605, 645-650
  SaoView view{ R + plane, V + plane, D + plane, fw, n, lx * n, ly * n, lx == g.wl - 1, ly == g.hl - 1, color ? 1 : 3 };
  for (int i = threadIdx.x; i < NACC * COPIES; i += 256) acc[i] = 0;
  const int copy = threadIdx.x & (COPIES - 1);
  for (int p = threadIdx.x; p < bw * bh; p += 256) {
    const int x = p % bw, y = p / bw;
    s_rec[p] = (u8)view.at(x, y);
    s_org[p] = src[plane + (long)(ly * n + y) * fw + lx * n + x];
  }
  __syncthreads();
  for (int p = threadIdx.x; p < bw * bh; p += 256) {
    const int x = p % bw, y = p / bw, c = s_rec[p], diff = (int)s_org[p] - c;
    const unsigned long long add = ((unsigned long long)(long long)diff << 32) + 1ull;  // sum += diff (two's complement in the high half), count += 1
    atomicAdd(&acc[(20 + (c >> 3)) * COPIES + copy], add);
    if (x >= 1 && x < bw - 1 && y >= 1 && y < bh - 1) {  // sao-generic.c:68-69: the block's interior
#pragma unroll
      for (int ec = 0; ec < 4; ec++) {
        int ax, ay, bx, by;
        eo_offsets(ec, ax, ay, bx, by);
        const int cat = eo_cat(s_rec[p + ay * bw + ax], s_rec[p + by * bw + bx], c);
        if (cat) atomicAdd(&acc[(ec * 5 + cat) * COPIES + copy], add);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 4 * 5 + 32) {  // unpack: the low half's carries never reach bit 32 (counts <= 4096), the high half is the signed sum
    unsigned long long v = 0;
    for (int k = 0; k < COPIES; k++) v += acc[threadIdx.x * COPIES + k];
    const i32 sum = (i32)(v >> 32), cnt = (i32)(v & 0xffffffffu);
    if (threadIdx.x < 20) { st.edge_sum[threadIdx.x / 5][threadIdx.x % 5] = sum; st.edge_cnt[threadIdx.x / 5][threadIdx.x % 5] = cnt; }
    else { st.band_sum[threadIdx.x - 20] = sum; st.band_cnt[threadIdx.x - 20] = cnt; }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < (int)(sizeof(SaoStats) / sizeof(i32)); i += 256) reinterpret_cast<i32 *>(&stats[item])[i] = reinterpret_cast<const i32 *>(&st)[i];
  if (threadIdx.x == 0) {
    SaoCand c;
    sao_candidates(st, c);
    cand[item] = c;
  }
}
// what the SAO decision takes from a picture's QP: lambda (pow stays on the host) and the two context states it prices with.  kvz_hip_dev_loop_filters_inter_pictures
// builds a row per QP 0 .. 51 and the kernel indexes it by the picture's QP
struct SaoQpRow { double lambda; int init_merge, init_type; };
// ... and the chain over the LCUs of a picture: one lane per picture
__global__ void __launch_bounds__(64) dev_sao_chain_kernel(const SaoStats *stats, const SaoCand *cand, const SaoGeom g, const int n_frames, const float *fbits, const Tables *tb,
                                                           const double lambda, const int init_merge, const int init_type, const int no_wpp, SaoRec *recs, u8 *merge,
                                                           const CtuModelTable pm = CtuModelTable(), const SaoQpRow *qp_rows = nullptr, const int32_t *qp_of_picture = nullptr)
{
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= n_frames) return;
  const long base = (long)f * g.wl * g.hl;
  if (qp_rows) {  // inter pictures with QPs of their own
    const SaoQpRow r = qp_rows[qp_of_picture[f]];
    sao_chain_picture(fbits, tb->ctx_next[0], tb->ctx_next[1], r.lambda, (u8)r.init_merge, (u8)r.init_type, no_wpp, g.wl, g.hl, stats + base * 3, cand + base * 3, recs + base * 3,
                      merge + base);
    return;
  }
  if (pm.models) {  // the picture's own lambda and SAO context states, from its row of the model table (kvz_hip_batch_loop_filters_models)
    const CtuModel *m = picture_model(pm, f);
    sao_chain_picture(fbits, tb->ctx_next[0], tb->ctx_next[1], m->lambda, m->ctx_init[KVZ_HIP_CX_SAO_MERGE], m->ctx_init[KVZ_HIP_CX_SAO_TYPE], no_wpp, g.wl, g.hl, stats + base * 3, cand + base * 3,
                      recs + base * 3, merge + base);
    return;
  }
  sao_chain_picture(fbits, tb->ctx_next[0], tb->ctx_next[1], lambda, (u8)init_merge, (u8)init_type, no_wpp, g.wl, g.hl, stats + base * 3, cand + base * 3, recs + base * 3,
                    merge + base);
}
// ... with a cost model per CTU (kvz_hip_batch_loop_filters_ctu_models): every LCU under its own lambda, the two contexts from the picture's slice model
__global__ void __launch_bounds__(64) dev_sao_chain_kernel_ctu(const SaoStats *stats, const SaoCand *cand, const SaoGeom g, const int n_frames, const float *fbits, const Tables *tb,
                                                               const int no_wpp, SaoRec *recs, u8 *merge, const CtuModelTable pm, const double *lambda_of_ctu)
{
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= n_frames) return;
  const long base = (long)f * g.wl * g.hl;
  const CtuModel *m = picture_model(pm, f);
  sao_chain_picture(fbits, tb->ctx_next[0], tb->ctx_next[1], m->lambda, m->ctx_init[KVZ_HIP_CX_SAO_MERGE], m->ctx_init[KVZ_HIP_CX_SAO_TYPE], no_wpp, g.wl, g.hl, stats + base * 3, cand + base * 3,
                    recs + base * 3, merge + base, lambda_of_ctu + base);
}

}  // namespace kvz
#include "kvz_fme.hpp"
#include "kvz_me.hpp"
#include "kvz_inter_kernels.hpp"
#include "kvz_inter_host.hpp"
#include "kvz_inter_joint.hpp"
#include "kvz_slice_contexts.hpp"

namespace kvz {
__global__ void dev_cu_dbk_kernel(const kvz_hip_cu_info *cu, int count, kvz_hip_cu_dbk *out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const kvz_hip_cu_info c = cu[i];
  kvz_hip_cu_dbk o;
  __builtin_memset(&o, 0, sizeof o);
  const unsigned masks[5] = { 0x1f, 0x0f, 0x07, 0x03, 0x1 };
  o.type = c.type; o.depth = c.depth; o.tr_depth = c.tr_depth; o.part_size = 0;
  o.cbf_y = (uint8_t)((c.cbf & masks[c.tr_depth > 4 ? 4 : c.tr_depth]) != 0);
  if (c.type == 2) {
    o.mv_dir = c.mv_dir;
    for (int l = 0; l < 2; l++) { o.mv_ref[l] = (int8_t)((c.mv_dir & (1 << l)) ? c.mv_ref[l] : 0); o.ref_id[l] = 0; o.mv[l][0] = c.mv[l][0]; o.mv[l][1] = c.mv[l][1]; }
  }
  out[i] = o;
}
// the device-side scratch of kvz_hip_dev_inter_ctu_pass, grown on demand and kept between calls
struct InterScratch {
  InterSlab *slabs = nullptr; int n_slabs = 0;
  ICtx *ctx = nullptr; unsigned *done = nullptr; uint32_t *items = nullptr; long n_ctus = 0;
  unsigned *ticket = nullptr;  // [0] ticket, [1] error
  void *model = nullptr; size_t model_bytes = 0;  // the launch's InterModel, or its picture table (InterFrames::pictures)
  void *lists = nullptr; size_t lists_bytes = 0;  // kvz_hip_dev_inter_ctu_pass_lists: the picture table with the factor rows behind it (kvz_inter_host.hpp
  std::vector<uint64_t> h_lists;                  // inter_picture_table_lists), grow-only, and what it holds: copied again only when a call's image differs
  uint8_t *entropy_table = nullptr; size_t entropy_table_bytes = 0;  // kvz_hip_dev_entropy_code_inter_pictures: context rows, POCs and rows of the pictures
  void *joint = nullptr; size_t joint_bytes = 0;  // kvz_hip_dev_inter_ctu_pass_groups: the table of the launch (kvz_inter_joint.hpp inter_joint_table), grow-only,
  std::vector<uint64_t> h_joint;                  // and what it holds: copied again only when a call's image differs
};
// One set per calling thread and device, like the stream the work is queued on (be() is thread_local): two threads, or two devices of one process, never share
// ticket / done / slab buffers, and a buffer is only ever freed by the thread whose (synchronised) stream used it.
// A worker thread that exits frees its sets (kvz_runtime.hpp ThreadState): registered the first time a thread asks for one.
inline InterScratch &inter_scratch()
{
  static thread_local InterScratch s[64];
  static thread_local bool registered = false;
  if (!registered) {
    registered = true;
    InterScratch *all = s;
    thread_state().cleanups.push_back([all]() {
      for (int d = 0; d < 64; d++) {
        InterScratch &x = all[d];
        if (!x.slabs && !x.ctx && !x.ticket) continue;
        (void)hipSetDevice(d);
        (void)hipFree(x.slabs); (void)hipFree(x.ctx); (void)hipFree(x.done); (void)hipFree(x.items); (void)hipFree(x.ticket); (void)hipFree(x.model); (void)hipFree(x.lists); (void)hipFree(x.entropy_table); (void)hipFree(x.joint);
        x = InterScratch();
      }
    });
  }
  return s[current_device() & 63];
}
}  // namespace kvz
namespace kvz {

// ---------------------------------------------------------------------------------------------------------------
// Picture-hash MD5 (nal.c:88-101 kvz_image_md5 -> nal-generic.c:41-55 per plane): a serial chain of 64-byte blocks per plane, so the batch
// brings the parallelism: one lane per (frame, plane).  Each lane streams its plane with 64-byte reads (one cache line per block).
__global__ void __launch_bounds__(64) dev_md5_kernel(const u8 *frames, const int W, const int H, const long n_planes, u8 *out /* [n_planes][16] */)
{
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n_planes) return;
  const long frame = i / 3;
  const int plane = (int)(i % 3);
  const long bytes = plane ? (long)(W >> 1) * (H >> 1) : (long)W * H;
  const u8 *p = frames + frame * ((long)W * H * 3 / 2) + (plane == 0 ? 0 : (plane == 1 ? (long)W * H : (long)W * H * 5 / 4));
  u32 st[4] = { 0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u };
  md5_run(st, p, bytes / 64, (int)(bytes % 64), 1, (unsigned long long)bytes);
  for (int k = 0; k < 16; k++) out[i * 16 + k] = (u8)(st[k >> 2] >> (8 * (k & 3)));
}

// timing events per calling thread and device (an event belongs to the device it was created on)
struct DevTimer { hipEvent_t e0 = nullptr, e1 = nullptr; };
static DevTimer &thread_timer(int which)
{
  static thread_local DevTimer t[2][64];
  static thread_local bool registered = false;
  if (!registered) {
    registered = true;
    DevTimer *all = &t[0][0];
    thread_state().cleanups.push_back([all]() {
      for (int i = 0; i < 128; i++) if (all[i].e0) { (void)hipSetDevice(i & 63); (void)hipEventDestroy(all[i].e0); (void)hipEventDestroy(all[i].e1); all[i] = DevTimer(); }
    });
  }
  return t[which][current_device() & 63];
}
static DevTimer &dev_timer() { return thread_timer(0); }
static DevTimer &inter_timer() { return thread_timer(1); }
static float &inter_kernel_ms() { static thread_local float ms = 0; return ms; }
static int &inter_share() { static thread_local int parts = 1; return parts; }  // kvz_hip_dev_inter_set_share  // the last inter CTU pass's kernel, HIP events on its stream

}  // namespace kvz

// ---- assembling a picture from tile pictures (the receive side of the sharded inter configuration's exchange, kvazaar_amd/sharding.py) ----
// Every tile arrives as its own planar Y|U|V picture in a fixed-size slot; one launch pastes all of them into the full planar frame.  One workgroup per
// (tile, row of any plane): a row is w or w/2 contiguous bytes on both sides, copied sixteen bytes per lane where both ends are 16-byte aligned.
namespace kvz {
struct PasteTable { int n; int x[64], y[64], w[64], h[64], slot[64]; };
__global__ void __launch_bounds__(256) dev_paste_tiles_kernel(u8 *frame, const int W, const int H, const u8 *slots, const long slot_bytes, const PasteTable tb)
{
  const int ti = blockIdx.y;
  const int x = tb.x[ti], y = tb.y[ti], w = tb.w[ti], h = tb.h[ti];
  const u8 *src0 = slots + (long)tb.slot[ti] * slot_bytes;
  for (int row = blockIdx.x; row < 2 * h; row += gridDim.x) {  // h luma rows, then h/2 of U, h/2 of V
    const int plane = row < h ? 0 : (row < h + h / 2 ? 1 : 2), r = plane == 0 ? row : (plane == 1 ? row - h : row - h - h / 2);
    const int pw = plane ? w >> 1 : w, fw = plane ? W >> 1 : W;
    const u8 *src = src0 + (plane == 0 ? 0 : (plane == 1 ? (long)w * h : (long)w * h + (long)(w >> 1) * (h >> 1))) + (long)r * pw;
    u8 *dst = frame + (plane == 0 ? 0 : (plane == 1 ? (long)W * H : (long)W * H + (long)(W >> 1) * (H >> 1))) + (long)((plane ? y >> 1 : y) + r) * fw + (plane ? x >> 1 : x);
    if ((((unsigned long long)src | (unsigned long long)dst | (unsigned)pw) & 15) == 0) {
      for (int i = threadIdx.x * 16; i < pw; i += 256 * 16) *reinterpret_cast<uint4 *>(dst + i) = *reinterpret_cast<const uint4 *>(src + i);
    } else {
      for (int i = threadIdx.x; i < pw; i += 256) dst[i] = src[i];
    }
  }
}
}  // namespace kvz

extern "C" {

void *kvz_hip_dev_alloc(size_t bytes)
{
  kvz::runtime_init(-1);
  void *p = nullptr;
  KVZ_HIP_CHECK(hipMalloc(&p, bytes ? bytes : 1));
  return p;
}
void kvz_hip_dev_free(void *p) { if (p) KVZ_HIP_CHECK(hipFree(p)); }
void kvz_hip_dev_upload(void *d, const void *h, size_t n)
{
  KVZ_HIP_CHECK(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, be().stream));
  KVZ_HIP_CHECK(hipStreamSynchronize(be().stream));
}
void kvz_hip_dev_download(void *h, const void *d, size_t n)
{
  KVZ_HIP_CHECK(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, be().stream));
  KVZ_HIP_CHECK(hipStreamSynchronize(be().stream));
}
void kvz_hip_dev_sync(void) { KVZ_HIP_CHECK(hipStreamSynchronize(be().stream)); }
void kvz_hip_dev_copy(void *d, const void *s, size_t n) { KVZ_HIP_CHECK(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, be().stream)); }
void kvz_hip_dev_timer_start(void)
{
  kvz::DevTimer &t = kvz::dev_timer();
  if (!t.e0) { KVZ_HIP_CHECK(hipEventCreate(&t.e0)); KVZ_HIP_CHECK(hipEventCreate(&t.e1)); }
  KVZ_HIP_CHECK(hipEventRecord(t.e0, be().stream));
}
float kvz_hip_dev_timer_stop(void)
{
  kvz::DevTimer &t = kvz::dev_timer();
  float ms = 0;
  KVZ_HIP_CHECK(hipEventRecord(t.e1, be().stream));
  KVZ_HIP_CHECK(hipEventSynchronize(t.e1));
  KVZ_HIP_CHECK(hipEventElapsedTime(&ms, t.e0, t.e1));
  return ms;
}

#define KVZ_DEV_LAUNCH(kernel, items, ...)                                                                        \
  do {                                                                                                            \
    const long items_ = (items);                                                                                  \
    if (items_ > 0) {                                                                                             \
      hipLaunchKernelGGL(kernel, dim3((unsigned)((items_ + 255) / 256)), dim3(256), 0, be().stream, __VA_ARGS__); \
      KVZ_HIP_CHECK(hipGetLastError());                                                                           \
    }                                                                                                             \
  } while (0)

int kvz_hip_dev_sad_nxn(int n, const uint8_t *a, const uint8_t *b, int count, uint32_t *out)
{
  const long chunks = (long)count * n * n / 16;
  const uint4 *pa = reinterpret_cast<const uint4 *>(a), *pb = reinterpret_cast<const uint4 *>(b);
  switch (n) {
  case 8: KVZ_DEV_LAUNCH(kvz::dev_sad_kernel<8>, chunks, pa, pb, chunks, out); break;
  case 16: KVZ_DEV_LAUNCH(kvz::dev_sad_kernel<16>, chunks, pa, pb, chunks, out); break;
  case 32: KVZ_DEV_LAUNCH(kvz::dev_sad_kernel<32>, chunks, pa, pb, chunks, out); break;
  case 64:
    KVZ_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)count * sizeof(uint32_t), be().stream));
    KVZ_DEV_LAUNCH(kvz::dev_sad_kernel<64>, chunks, pa, pb, chunks, out);
    break;
  default: fprintf(stderr, "kvz_hip_dev_sad_nxn: unsupported n=%d\n", n); return -1;
  }
  return 0;
}

int kvz_hip_dev_satd_nxn(int n, const uint8_t *a, const uint8_t *b, int count, uint32_t *out)
{
  const long tiles = n >= 8 ? (long)count * (n / 8) * (n / 8) : count;
  switch (n) {
  case 4: KVZ_DEV_LAUNCH(kvz::dev_satd4_kernel, tiles, a, b, tiles, out); break;
  case 8: KVZ_DEV_LAUNCH(kvz::dev_satd_kernel<8>, tiles, a, b, tiles, out); break;
  case 16: KVZ_DEV_LAUNCH(kvz::dev_satd_kernel<16>, tiles, a, b, tiles, out); break;
  case 32: KVZ_DEV_LAUNCH(kvz::dev_satd_kernel<32>, tiles, a, b, tiles, out); break;
  case 64: KVZ_DEV_LAUNCH(kvz::dev_satd_kernel<64>, tiles, a, b, tiles, out); break;
  default: fprintf(stderr, "kvz_hip_dev_satd_nxn: unsupported n=%d\n", n); return -1;
  }
  return 0;
}

int kvz_hip_dev_transform(int kind, const int16_t *in, int16_t *tmp, int16_t *out, int count, int use_matrix_cores)
{
  static const int sizes[5] = { 4, 8, 16, 32, 4 };
  const int inverse = kind >= KVZ_HIP_IDCT_4, idx = inverse ? kind - KVZ_HIP_IDCT_4 : kind, n = sizes[idx];
  if (use_matrix_cores == 2 && n == 16) {  // 16-point blocks, A/B: one lane per row on v_dot2_i32_i16 (4.9 / 4.4 TB/s forward / inverse against 5.1 / 5.0 TB/s on the matrix cores, four blocks per wavefront)
    const long rows = (long)count * 16;
    KVZ_DEV_LAUNCH(kvz::dev_transform_rows_kernel<16>, (rows + 511) / 512 * 256, in, out, rows, inverse, &kvz::device_tables()->pairs16[0][0][0]);
    return 0;
  }
  if (use_matrix_cores && (n == 16 || n == 32) && idx != 4) {
    if (n == 16) KVZ_DEV_LAUNCH(kvz::dev_transform_mfma_kernel<16>, ((long)count + 15) / 16 * 256, in, out, count, inverse, kvz::device_tables());  // four blocks per wavefront
    else KVZ_DEV_LAUNCH(kvz::dev_transform_mfma_kernel<32>, ((long)count + 3) / 4 * 256, in, out, count, inverse, kvz::device_tables());
    return 0;
  }
  if (use_matrix_cores == 1) {  // the small sizes run on the vector ALU (v_dot2_i32_i16); use_matrix_cores == 2 keeps the block-diagonal MFMA form for A/B
    const kvz::Tables *tb = kvz::device_tables();
    const int kind_sp = idx == 4 ? 2 : (n == 8 ? 1 : 0);
    const long rows = (long)count * n, threads = (rows + 1023) / 1024 * 256;
    if (n == 4) KVZ_DEV_LAUNCH(kvz::dev_transform_rows_kernel<4>, threads, in, out, rows, inverse, &tb->small_pairs[kind_sp][0][0][0]);
    else KVZ_DEV_LAUNCH(kvz::dev_transform_rows_kernel<8>, threads, in, out, rows, inverse, &tb->small_pairs[kind_sp][0][0][0]);
    return 0;
  }
  if (use_matrix_cores) {
    const kvz::Tables *tb = kvz::device_tables();
    const int kind_bd = idx == 4 ? 2 : (n == 8 ? 1 : 0), per_wave = 16 / n;
    const long threads = ((long)count + 4 * per_wave - 1) / (4 * per_wave) * 256;
    if (n == 4) KVZ_DEV_LAUNCH(kvz::dev_transform_small_mfma_kernel<4>, threads, in, out, count, inverse, tb->bd_i8[kind_bd][0], tb->bd_i8[kind_bd][1], tb->bd_sum[kind_bd][0], tb->bd_sum[kind_bd][1]);
    else KVZ_DEV_LAUNCH(kvz::dev_transform_small_mfma_kernel<8>, threads, in, out, count, inverse, tb->bd_i8[kind_bd][0], tb->bd_i8[kind_bd][1], tb->bd_sum[kind_bd][0], tb->bd_sum[kind_bd][1]);
    return 0;
  }
  if (!tmp) { fprintf(stderr, "kvz_hip_dev_transform: the scalar path needs tmp\n"); return -1; }
  A::transform_dev(be(), kind, 8, in, tmp, out, count);
  return 0;
}

int kvz_hip_dev_angular_pred(int log2_width, int mode, const uint8_t *ref_above, const uint8_t *ref_left, int count, uint8_t *out)
{
  if (count <= 0) return 0;
  const int blocks_per_wg = 256 * kvz::kAngularGroupsPerLane / ((1 << (2 * log2_width)) / 4);
  const long threads = ((long)count + blocks_per_wg - 1) / blocks_per_wg * 256;
  switch (log2_width) {
  case 2: KVZ_DEV_LAUNCH(kvz::dev_angular_kernel<2>, threads, ref_above, ref_left, count, mode, out); break;
  case 3: KVZ_DEV_LAUNCH(kvz::dev_angular_kernel<3>, threads, ref_above, ref_left, count, mode, out); break;
  case 4: KVZ_DEV_LAUNCH(kvz::dev_angular_kernel<4>, threads, ref_above, ref_left, count, mode, out); break;
  case 5: KVZ_DEV_LAUNCH(kvz::dev_angular_kernel<5>, threads, ref_above, ref_left, count, mode, out); break;
  default: fprintf(stderr, "kvz_hip_dev_angular_pred: unsupported log2_width=%d\n", log2_width); return -1;
  }
  return 0;
}

int kvz_hip_dev_intra_select(int log2w, int nblk, const uint32_t *raw, const int8_t *preds, const double *mode_bits, int count, int32_t *winner)
{
  if (!((log2w == 3 && nblk == 1) || (log2w == 4 && nblk == 4))) { fprintf(stderr, "kvz_hip_dev_intra_select: unsupported log2w=%d nblk=%d\n", log2w, nblk); return -1; }
  if (count <= 0) return 0;
  KVZ_DEV_LAUNCH(kvz::dev_intra_select_kernel, ((long)count + 3) / 4 * 256, raw, preds, mode_bits, count, log2w, nblk, winner);
  return 0;
}

int kvz_hip_dev_cu8_units(int count, int from_coeffs, const int16_t *in, const int32_t *qp, int16_t *levels, int16_t *dequant, int16_t *resid)
{
  if (count < 0 || (from_coeffs != 0 && from_coeffs != 1)) { fprintf(stderr, "kvz_hip_dev_cu8_units: count=%d from_coeffs=%d\n", count, from_coeffs); return -1; }
  if (count == 0) return 0;
  KVZ_DEV_LAUNCH(kvz::dev_cu8_units_kernel, ((long)count + 1) / 2 * 256, in, qp, count, from_coeffs, kvz::device_tables(), levels, dequant, resid);
  return 0;
}

int kvz_hip_dev_rough_rows(int log2w, const uint8_t *top, const uint8_t *left, int count, uint8_t *out)
{
  if (count < 0 || (log2w != 3 && log2w != 4)) { fprintf(stderr, "kvz_hip_dev_rough_rows: log2w=%d count=%d\n", log2w, count); return -1; }
  if (log2w == 3) KVZ_DEV_LAUNCH(kvz::dev_rough_rows_kernel<3>, ((long)count + 1) / 2 * 256, kvz::device_tables(), top, left, count, out);
  else KVZ_DEV_LAUNCH(kvz::dev_rough_rows_kernel<4>, ((long)count + 1) / 2 * 256, kvz::device_tables(), top, left, count, out);
  return 0;
}

int kvz_hip_dev_cu16_predict(const uint8_t *top, const uint8_t *left, const uint8_t *modes, int count, uint8_t *out)
{
  if (count < 0) { fprintf(stderr, "kvz_hip_dev_cu16_predict: count=%d\n", count); return -1; }
  KVZ_DEV_LAUNCH(kvz::dev_cu16_predict_kernel, ((long)count + 1) / 2 * 256, kvz::device_tables(), top, left, modes, count, out);
  return 0;
}

int kvz_hip_dev_satd8_blocks(const uint8_t *a, const uint8_t *b, int count, uint32_t *out)
{
  if (count < 0) { fprintf(stderr, "kvz_hip_dev_satd8_blocks: count=%d\n", count); return -1; }
  KVZ_DEV_LAUNCH(kvz::dev_satd8_blocks_kernel, ((long)count + 31) / 32 * 64, kvz::device_tables(), a, b, count, out);
  return 0;
}

void kvz_hip_dev_deblock_frames(uint8_t *frames, int width, int height, int n_frames, const uint8_t *cu_depth, int qp, int beta_offset_div2,
                                int tc_offset_div2)
{
  kvz::deblock_frames_on(be().stream, frames, width, height, n_frames, cu_depth, qp, beta_offset_div2, tc_offset_div2);
}

void kvz_hip_dev_deblock_frames_inter(uint8_t *frames, int width, int height, int n_frames, const kvz_hip_cu_dbk *info, int qp, int beta_offset_div2, int tc_offset_div2,
                                      int slice_is_b)
{
  kvz::deblock_frames_on(be().stream, frames, width, height, n_frames, nullptr, qp, beta_offset_div2, tc_offset_div2, 3, info, slice_is_b);
}

namespace kvz {
// kvz_hip_sao_params <-> the packed records (kvz_sao.hpp SaoRec), stated once for every host-side conversion: plane 0 is the luma structure, planes 1 and 2 are the
// chroma structure's slots 0 and 1 (band_position[slot], offsets[5 * slot ..]); type and eo_class are the structure's for both of its slots
inline SaoRec sao_rec_pack(const kvz_hip_sao_params &p, int slot)
{
  SaoRec r = (SaoRec)(p.type & 0xff) | ((SaoRec)(p.eo_class & 0xff) << 8) | ((SaoRec)(p.band_position[slot] & 0xff) << 16);
  for (int k = 0; k < 5; k++) r |= (SaoRec)(u8)(int8_t)p.offsets[5 * slot + k] << (24 + 8 * k);
  return r;
}
inline void sao_rec_unpack(SaoRec r, kvz_hip_sao_params *o, int slot)
{
  if (slot == 0) { memset(o, 0, sizeof *o); o->bitdepth = 8; o->type = (int)(r & 0xff); o->eo_class = (int)((r >> 8) & 0xff); }
  o->band_position[slot] = (int)((r >> 16) & 0xff);
  for (int k = 0; k < 5; k++) o->offsets[5 * slot + k] = (int)(int8_t)(r >> (24 + 8 * k));
}
// ... of a picture's LCUs: recs [lcus][3]; luma / chroma may be null
inline void sao_recs_unpack(const SaoRec *recs, size_t lcus, kvz_hip_sao_params *luma, kvz_hip_sao_params *chroma)
{
  for (size_t i = 0; i < lcus; i++) {
    if (luma) sao_rec_unpack(recs[i * 3], &luma[i], 0);
    if (chroma) { sao_rec_unpack(recs[i * 3 + 1], &chroma[i], 0); sao_rec_unpack(recs[i * 3 + 2], &chroma[i], 1); }
  }
}
}  // namespace kvz
// The loop filters between two pictures of a device-resident chain with inter prediction: kvz_hip_batch_loop_filters' pipeline (three pictures R / V / D, the
// statistics kernel, the decision chain, the SAO kernel) with the deblocking edges and strengths taken from kvz_hip_cu_dbk records.
namespace kvz {
struct LoopScratch {
  u8 *ver = nullptr, *dbk = nullptr; size_t pic_bytes = 0;
  SaoStats *stats = nullptr; SaoCand *cand = nullptr; SaoRec *recs = nullptr; u8 *merge = nullptr; size_t lcus = 0;
  float *fbits = nullptr;
  int32_t *qps = nullptr; size_t n_qps = 0;  // kvz_hip_dev_loop_filters_inter_pictures: the pictures' QPs
  SaoQpRow *sao_rows = nullptr;              // ... and the SAO decision's row per QP 0 .. 51
};
// per calling thread and device (see inter_scratch): kvz_hip_dev_entropy_code_inter reads the SAO decisions the LAST kvz_hip_dev_loop_filters_inter of the same thread
// left on the same device
inline LoopScratch &loop_scratch()
{
  static thread_local LoopScratch s[64];
  static thread_local bool registered = false;
  if (!registered) {
    registered = true;
    LoopScratch *all = s;
    thread_state().cleanups.push_back([all]() {
      for (int d = 0; d < 64; d++) {
        LoopScratch &x = all[d];
        if (!x.ver && !x.stats && !x.fbits) continue;
        (void)hipSetDevice(d);
        (void)hipFree(x.ver); (void)hipFree(x.dbk); (void)hipFree(x.stats); (void)hipFree(x.cand); (void)hipFree(x.recs); (void)hipFree(x.merge); (void)hipFree(x.fbits); (void)hipFree(x.qps); (void)hipFree(x.sao_rows);
        x = LoopScratch();
      }
    });
  }
  return s[current_device() & 63];
}
}  // namespace kvz
// kvz_hip_dev_loop_filters_inter (qp_host == nullptr: `qp` for every picture) and kvz_hip_dev_loop_filters_inter_pictures (qp_host: a checked HOST array, `qp` unused);
// slice_type: KVZ_HIP_SLICE_B, _P or _I -- slice_is_b != 0 is B, slice_is_b == 0 has always been I
static int kvz_loop_filters_inter_run(const uint8_t *src, uint8_t *rec, int width, int height, int n_pictures, const kvz_hip_cu_dbk *info, int qp, const int32_t *qp_host, int slice_type,
                                      int deblock, int beta_offset_div2, int tc_offset_div2, int sao, int no_wpp, kvz_hip_sao_params *luma, kvz_hip_sao_params *chroma, uint8_t *merge);
int kvz_hip_dev_loop_filters_inter(const uint8_t *src, uint8_t *rec, int width, int height, int n_pictures, const kvz_hip_cu_dbk *info, int qp, int slice_is_b, int deblock,
                                   int beta_offset_div2, int tc_offset_div2, int sao, int no_wpp, kvz_hip_sao_params *luma, kvz_hip_sao_params *chroma, uint8_t *merge)
{
  if (n_pictures <= 0) return 0;
  if (!src || !rec || !info || width <= 0 || height <= 0 || (width & 7) || (height & 7) || qp < 0 || qp > 51) { fprintf(stderr, "kvz_hip_dev_loop_filters_inter: bad argument\n"); return -1; }
  return kvz_loop_filters_inter_run(src, rec, width, height, n_pictures, info, qp, nullptr, slice_is_b ? KVZ_HIP_SLICE_B : KVZ_HIP_SLICE_I, deblock, beta_offset_div2, tc_offset_div2, sao, no_wpp, luma, chroma, merge);
}
int kvz_hip_dev_loop_filters_inter_pictures(const uint8_t *src, uint8_t *rec, int width, int height, int n_pictures, const kvz_hip_cu_dbk *info, const int32_t *qp_of_picture,
                                            int slice_is_b, int deblock, int beta_offset_div2, int tc_offset_div2, int sao, int no_wpp, kvz_hip_sao_params *luma,
                                            kvz_hip_sao_params *chroma, uint8_t *merge)
{
  if (n_pictures <= 0) return 0;
  if (!src || !rec || !info || width <= 0 || height <= 0 || (width & 7) || (height & 7)) { fprintf(stderr, "kvz_hip_dev_loop_filters_inter_pictures: bad argument\n"); return -1; }
  if (!kvz::inter_picture_qps_known(qp_of_picture, n_pictures, "kvz_hip_dev_loop_filters_inter_pictures")) return -1;
  return kvz_loop_filters_inter_run(src, rec, width, height, n_pictures, info, 0, qp_of_picture, slice_is_b ? KVZ_HIP_SLICE_B : KVZ_HIP_SLICE_I, deblock, beta_offset_div2, tc_offset_div2, sao, no_wpp, luma, chroma, merge);
}
// ... with the slice type named (kvz_hip_dev.h): P is deblocked as every slice that is not B is (filter.c:428), its SAO decision starts from the P row's states
int kvz_hip_dev_loop_filters_inter_slices(const uint8_t *src, uint8_t *rec, int width, int height, int n_pictures, const kvz_hip_cu_dbk *info, int qp, const int32_t *qp_of_picture,
                                          int slice_type, int deblock, int beta_offset_div2, int tc_offset_div2, int sao, int no_wpp, kvz_hip_sao_params *luma,
                                          kvz_hip_sao_params *chroma, uint8_t *merge)
{
  if (n_pictures <= 0) return 0;
  if (slice_type != KVZ_HIP_SLICE_B && slice_type != KVZ_HIP_SLICE_P && slice_type != KVZ_HIP_SLICE_I) {
    fprintf(stderr, "kvz_hip_dev_loop_filters_inter_slices: slice type %d is none of KVZ_HIP_SLICE_B (0), KVZ_HIP_SLICE_P (1), KVZ_HIP_SLICE_I (2)\n", slice_type);
    return -1;
  }
  if (!src || !rec || !info || width <= 0 || height <= 0 || (width & 7) || (height & 7) || (!qp_of_picture && (qp < 0 || qp > 51))) { fprintf(stderr, "kvz_hip_dev_loop_filters_inter_slices: bad argument\n"); return -1; }
  if (qp_of_picture && !kvz::inter_picture_qps_known(qp_of_picture, n_pictures, "kvz_hip_dev_loop_filters_inter_slices")) return -1;
  return kvz_loop_filters_inter_run(src, rec, width, height, n_pictures, info, qp_of_picture ? 0 : qp, qp_of_picture, slice_type, deblock, beta_offset_div2, tc_offset_div2, sao, no_wpp, luma, chroma, merge);
}
// ... of P pictures with reference lists (kvz_hip_dev.h): a thin form.  A P slice has one list, so two reference indices name the same picture exactly when they are
// equal, and that is what dbk_strength compares for a slice that is not B: the kernels need nothing new.  refs == NULL is kvz_hip_dev_loop_filters_inter_slices; with
// refs the table is checked (the filters read no POC, so the order of the POCs is not) and the slice type must be P
int kvz_hip_dev_loop_filters_inter_refs(const uint8_t *src, uint8_t *rec, int width, int height, int n_pictures, const kvz_hip_cu_dbk *info, int qp, const int32_t *qp_of_picture,
                                        int slice_type, int deblock, int beta_offset_div2, int tc_offset_div2, int sao, int no_wpp, kvz_hip_sao_params *luma,
                                        kvz_hip_sao_params *chroma, uint8_t *merge, const kvz_hip_inter_refs *refs)
{
  if (n_pictures <= 0) return 0;
  if (refs && slice_type != KVZ_HIP_SLICE_B && slice_type != KVZ_HIP_SLICE_P && slice_type != KVZ_HIP_SLICE_I) {
    fprintf(stderr, "kvz_hip_dev_loop_filters_inter_refs: slice type %d is none of KVZ_HIP_SLICE_B (0), KVZ_HIP_SLICE_P (1), KVZ_HIP_SLICE_I (2)\n", slice_type);
    return -1;
  }
  if (!kvz::inter_refs_launch_known(refs, n_pictures, true, nullptr, slice_type, "kvz_hip_dev_loop_filters_inter_refs")) return -1;
  return kvz_hip_dev_loop_filters_inter_slices(src, rec, width, height, n_pictures, info, qp, qp_of_picture, slice_type, deblock, beta_offset_div2, tc_offset_div2, sao, no_wpp, luma, chroma, merge);
}
static int kvz_loop_filters_inter_run(const uint8_t *src, uint8_t *rec, int width, int height, int n_pictures, const kvz_hip_cu_dbk *info, int qp, const int32_t *qp_host, int slice_type,
                                      int deblock, int beta_offset_div2, int tc_offset_div2, int sao, int no_wpp, kvz_hip_sao_params *luma, kvz_hip_sao_params *chroma, uint8_t *merge)
{
  const int slice_is_b = slice_type == KVZ_HIP_SLICE_B;  // what the deblocking kernels ask
  hipStream_t st = be().stream;
  const int32_t *qps = nullptr;  // device: the pictures' QPs
  if (qp_host) {
    kvz::LoopScratch &lq = kvz::loop_scratch();
    if ((size_t)n_pictures > lq.n_qps) {
      if (lq.qps) KVZ_HIP_CHECK(hipFree(lq.qps));
      KVZ_HIP_CHECK(hipMalloc((void **)&lq.qps, (size_t)n_pictures * sizeof(int32_t)));
      lq.n_qps = (size_t)n_pictures;
    }
    KVZ_HIP_CHECK(hipMemcpyAsync(lq.qps, qp_host, (size_t)n_pictures * sizeof(int32_t), hipMemcpyHostToDevice, st));
    KVZ_HIP_CHECK(hipStreamSynchronize(st));  // the caller's array
    qps = lq.qps;
  }
  if (!sao) {
    if (deblock) kvz::deblock_frames_on(st, rec, width, height, n_pictures, nullptr, qp, beta_offset_div2, tc_offset_div2, 3, info, slice_is_b, qps);
    return 0;
  }
  const int wc = (width + 63) >> 6, hc = (height + 63) >> 6;
  const long frame_px = (long)width * height * 3 / 2;
  const size_t pic_bytes = (size_t)frame_px * n_pictures, lcus = (size_t)wc * hc * n_pictures;
  kvz::LoopScratch &sc = kvz::loop_scratch();
  if (pic_bytes > sc.pic_bytes) {
    if (sc.ver) { KVZ_HIP_CHECK(hipFree(sc.ver)); KVZ_HIP_CHECK(hipFree(sc.dbk)); }
    KVZ_HIP_CHECK(hipMalloc((void **)&sc.ver, pic_bytes));
    KVZ_HIP_CHECK(hipMalloc((void **)&sc.dbk, pic_bytes));
    sc.pic_bytes = pic_bytes;
  }
  if (lcus > sc.lcus) {
    if (sc.stats) { KVZ_HIP_CHECK(hipFree(sc.stats)); KVZ_HIP_CHECK(hipFree(sc.cand)); KVZ_HIP_CHECK(hipFree(sc.recs)); KVZ_HIP_CHECK(hipFree(sc.merge)); }
    KVZ_HIP_CHECK(hipMalloc((void **)&sc.stats, lcus * 3 * sizeof(kvz::SaoStats)));
    KVZ_HIP_CHECK(hipMalloc((void **)&sc.cand, lcus * 3 * sizeof(kvz::SaoCand)));
    KVZ_HIP_CHECK(hipMalloc((void **)&sc.recs, lcus * 3 * sizeof(kvz::SaoRec)));
    KVZ_HIP_CHECK(hipMalloc((void **)&sc.merge, lcus));
    sc.lcus = lcus;
  }
  if (!sc.fbits) {
    float fbits[128];
    for (int i = 0; i < 128; i++) fbits[i] = (float)kvz::kEntropyBits[i] / 32768.0f;
    KVZ_HIP_CHECK(hipMalloc((void **)&sc.fbits, sizeof fbits));
    KVZ_HIP_CHECK(hipMemcpy(sc.fbits, fbits, sizeof fbits, hipMemcpyHostToDevice));
  }
  // R = rec (kept until the SAO kernel has read D), V = after the vertical edges, D = after all edges (sao.c:632-735 reads all three around an LCU's borders)
  KVZ_HIP_CHECK(hipMemcpyAsync(sc.ver, rec, pic_bytes, hipMemcpyDeviceToDevice, st));
  if (deblock) kvz::deblock_frames_on(st, sc.ver, width, height, n_pictures, nullptr, qp, beta_offset_div2, tc_offset_div2, 1, info, slice_is_b, qps);
  KVZ_HIP_CHECK(hipMemcpyAsync(sc.dbk, sc.ver, pic_bytes, hipMemcpyDeviceToDevice, st));
  if (deblock) kvz::deblock_frames_on(st, sc.dbk, width, height, n_pictures, nullptr, qp, beta_offset_div2, tc_offset_div2, 2, info, slice_is_b, qps);
  const kvz::SaoGeom g{ width, height, wc, hc, frame_px };
  // rate_control.c:678-691 at the picture's QP; context.c:38-39 INIT_SAO_MERGE_FLAG / INIT_SAO_TYPE_IDX of the slice type (B: 153 / 160, P: 153 / 185, I: 153 / 200)
  auto sao_row = [&](int q) { return kvz::SaoQpRow{ 0.57 * pow(2.0, (q - 12) / 3.0), kvz::ctx_state(q, 153), kvz::ctx_state(q, kvz::sao_type_init_value(slice_type)) }; };
  const kvz::SaoQpRow row = sao_row(qp);
  const double lambda = row.lambda;
  const int cx_merge = row.init_merge, cx_type = row.init_type;
  if (qps) {  // a row per QP: the kernel takes the picture's
    kvz::SaoQpRow rows[52];
    for (int q = 0; q < 52; q++) rows[q] = sao_row(q);
    if (!sc.sao_rows) KVZ_HIP_CHECK(hipMalloc((void **)&sc.sao_rows, sizeof rows));
    KVZ_HIP_CHECK(hipMemcpyAsync(sc.sao_rows, rows, sizeof rows, hipMemcpyHostToDevice, st));
    KVZ_HIP_CHECK(hipStreamSynchronize(st));  // `rows` is a stack object
  }
  hipLaunchKernelGGL(kvz::dev_sao_stats_kernel, dim3((unsigned)(lcus * 3)), dim3(256), 0, st, src, rec, sc.ver, sc.dbk, g, sc.stats, sc.cand);
  hipLaunchKernelGGL(kvz::dev_sao_chain_kernel, dim3((unsigned)((n_pictures + 63) / 64)), dim3(64), 0, st, (const kvz::SaoStats *)sc.stats, (const kvz::SaoCand *)sc.cand, g, n_pictures, sc.fbits,
                     kvz::device_tables(), lambda, cx_merge, cx_type, no_wpp, sc.recs, sc.merge, kvz::CtuModelTable(), qps ? (const kvz::SaoQpRow *)sc.sao_rows : nullptr, qps);
  kvz::launch_sao(st, sc.dbk, rec, width, height, n_pictures, sc.recs, nullptr, nullptr);
  KVZ_HIP_CHECK(hipGetLastError());
  if (luma || chroma || merge) {  // host copies of the decisions (what the encoder writes as SAO syntax)
    std::vector<kvz::SaoRec> recs(lcus * 3);
    KVZ_HIP_CHECK(hipMemcpyAsync(recs.data(), sc.recs, lcus * 3 * sizeof(kvz::SaoRec), hipMemcpyDeviceToHost, st));
    if (merge) KVZ_HIP_CHECK(hipMemcpyAsync(merge, sc.merge, lcus, hipMemcpyDeviceToHost, st));
    KVZ_HIP_CHECK(hipStreamSynchronize(st));
    kvz::sao_recs_unpack(recs.data(), lcus, luma, chroma);
  }
  return 0;
}

int kvz_hip_dev_sad_surface(const uint8_t *cur, const uint8_t *ref, int width, int height, int bw, int range, const int16_t *blk_xy, int count,
                             uint32_t *out)
{
  if (count <= 0) return 0;
  if (range < 0 || range > 32) { fprintf(stderr, "kvz_hip_dev_sad_surface: range %d not in [0, 32]\n", range); return -1; }
  const dim3 grid((unsigned)count), block(kvz::kSadSurfaceLanes);
  switch (bw) {
  case 8: hipLaunchKernelGGL(kvz::dev_sad_surface_kernel<8>, grid, block, 0, be().stream, cur, ref, width, height, range, blk_xy, out); break;
  case 16: hipLaunchKernelGGL(kvz::dev_sad_surface_kernel<16>, grid, block, 0, be().stream, cur, ref, width, height, range, blk_xy, out); break;
  case 32: hipLaunchKernelGGL(kvz::dev_sad_surface_kernel<32>, grid, block, 0, be().stream, cur, ref, width, height, range, blk_xy, out); break;
  case 64: hipLaunchKernelGGL(kvz::dev_sad_surface_kernel<64>, grid, block, 0, be().stream, cur, ref, width, height, range, blk_xy, out); break;
  default: fprintf(stderr, "kvz_hip_dev_sad_surface: unsupported block width %d\n", bw); return -1;
  }
  KVZ_HIP_CHECK(hipGetLastError());
  return 0;
}

int kvz_hip_dev_fme_costs(const uint8_t *cur, const uint8_t *ref, int width, int height, const kvz_hip_fme_pu *pus, int count, int max_pu_size, int steps, uint32_t *out)
{
  if (count <= 0) return 0;
  const dim3 grid((unsigned)count), block(256);
  const kvz::Tables *tb = kvz::device_tables();
  if (max_pu_size <= 16) hipLaunchKernelGGL(kvz::dev_fme_kernel<16>, grid, block, 0, be().stream, cur, ref, width, height, pus, steps, tb, out);
  else if (max_pu_size <= 32) hipLaunchKernelGGL(kvz::dev_fme_kernel<32>, grid, block, 0, be().stream, cur, ref, width, height, pus, steps, tb, out);
  else if (max_pu_size <= 64) hipLaunchKernelGGL(kvz::dev_fme_kernel<64>, grid, block, 0, be().stream, cur, ref, width, height, pus, steps, tb, out);
  else { fprintf(stderr, "kvz_hip_dev_fme_costs: PUs larger than 64 samples do not exist\n"); return -1; }
  KVZ_HIP_CHECK(hipGetLastError());
  return 0;
}

void kvz_hip_dev_cu_dbk_from_info(const kvz_hip_cu_info *cu, int count, kvz_hip_cu_dbk *out)
{
  if (count <= 0) return;
  hipLaunchKernelGGL(kvz::dev_cu_dbk_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, be().stream, cu, count, out);
  KVZ_HIP_CHECK(hipGetLastError());
}

int kvz_hip_dev_inter_ctu_pass(const uint8_t *src, const uint8_t *ref, const kvz_hip_cu_info *ref_cu, uint8_t *rec, kvz_hip_cu_info *cu, int16_t *coeff, int width,
                               int height, int n_pictures, const kvz_hip_inter_params *p)
{
  return kvz_hip_dev_inter_ctu_pass_tiles(src, ref, ref_cu, rec, cu, coeff, width, height, n_pictures, p, nullptr, 0);
}
int kvz_hip_dev_inter_ctu_pass_tiles(const uint8_t *src, const uint8_t *ref, const kvz_hip_cu_info *ref_cu, uint8_t *rec, kvz_hip_cu_info *cu, int16_t *coeff, int width,
                                     int height, int n_pictures, const kvz_hip_inter_params *p, const int32_t *tile_xy, int n_references)
{
  return kvz_hip_dev_inter_ctu_pass_pictures(src, ref, ref_cu, rec, cu, coeff, width, height, n_pictures, p, tile_xy, n_references, nullptr);
}
int kvz_hip_dev_inter_ctu_pass_pictures(const uint8_t *src, const uint8_t *ref, const kvz_hip_cu_info *ref_cu, uint8_t *rec, kvz_hip_cu_info *cu, int16_t *coeff, int width,
                                        int height, int n_pictures, const kvz_hip_inter_params *p, const int32_t *tile_xy, int n_references,
                                        const kvz_hip_inter_pictures *pictures)
{
  return kvz_hip_dev_inter_ctu_pass_lists(src, ref, ref_cu, rec, cu, coeff, width, height, n_pictures, p, tile_xy, n_references, pictures, nullptr, 0, nullptr);
}
// ---- what the launches of the inter CTU pass share (kvz_inter_ctu_pass_run, kvz_hip_dev_inter_ctu_pass_groups): the scratch, the grid, and the launch itself ----
namespace kvz {
// the scratch per CTU of a launch of `total` CTUs (context output, `done` flags, ticket list) and the ticket / error words: grow-only
static void inter_scratch_reserve(InterScratch &sc, long total)
{
  if (total > sc.n_ctus) {
    if (sc.ctx) { KVZ_HIP_CHECK(hipFree(sc.ctx)); KVZ_HIP_CHECK(hipFree(sc.done)); KVZ_HIP_CHECK(hipFree(sc.items)); }
    KVZ_HIP_CHECK(hipMalloc((void **)&sc.ctx, (size_t)total * sizeof(ICtx)));
    KVZ_HIP_CHECK(hipMalloc((void **)&sc.done, (size_t)total * sizeof(unsigned)));
    KVZ_HIP_CHECK(hipMalloc((void **)&sc.items, (size_t)total * sizeof(uint32_t)));
    sc.n_ctus = total;
  }
  if (!sc.ticket) KVZ_HIP_CHECK(hipMalloc((void **)&sc.ticket, 2 * sizeof(unsigned)));
}
// The persistent grid of a launch of `total` CTUs under the build of `unit` (kvz_inter_builds.hpp), one workgroup per slot, with a slab for each: resident workgroups
// (= wavefronts) per CU times the CUs, clamped to the work.  What THIS build's registers and LDS allow is the ceiling: a share (kvz_hip_dev_inter_set_share, per
// calling thread) divides it, the developer's environment value is clamped to it.  n_groups: of a joint launch, for the KVZ_HIP_INTER_VERBOSE line
static int inter_grid(InterScratch &sc, int unit, long total, int n_groups = 0)
{
  int dev_id = 0, n_cu = 256, fit = 0;
  KVZ_HIP_CHECK(hipGetDevice(&dev_id));
  KVZ_HIP_CHECK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev_id));
  KVZ_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, inter_build_kernel(unit), KVZ_ICTU_THREADS, 0));
  if (fit <= 0) fit = 8;
  const char *env = getenv("KVZ_HIP_INTER_WG_PER_CU");
  int per_cu = fit / inter_share();
  if (env && atoi(env) > 0) per_cu = atoi(env) < fit ? atoi(env) : fit;
  if (per_cu < 1) per_cu = 1;
  int n_wg = n_cu * per_cu;
  if (getenv("KVZ_HIP_INTER_VERBOSE")) {  // the build by its words: the suffix of the kernel's name, spaced
    char words[32], groups[32] = "";
    snprintf(words, sizeof words, "%s", inter_build_suffix(unit));
    for (char *c = words; *c; c++) if (*c == '_') *c = ' ';
    if (n_groups) snprintf(groups, sizeof groups, "%d groups, ", n_groups);
    fprintf(stderr, "kvz_hip inter pass: %s build, %s%d workgroups per CU x %d CUs\n", words, groups, per_cu, n_cu);
  }
  if ((long)n_wg > total) n_wg = (int)total;
  if (n_wg > sc.n_slabs) {
    if (sc.slabs) KVZ_HIP_CHECK(hipFree(sc.slabs));
    KVZ_HIP_CHECK(hipMalloc((void **)&sc.slabs, (size_t)n_wg * sizeof(InterSlab)));
    sc.n_slabs = n_wg;
  }
  return n_wg;
}
// The launch, timed by the events of inter_kernel_ms(): F.ctx_out / F.slabs and the schedule are the scratch's, whose ticket list the caller has uploaded and whose
// `done` flags and ticket / error words it has zeroed.  Returns when the kernel has ended: 0, or -2 when it raised its error word
static int inter_launch(InterScratch &sc, int unit, int n_wg, InterFrames F, const InterModel *d_model, long total, int no_wpp, hipStream_t st)
{
  F.ctx_out = sc.ctx; F.slabs = sc.slabs;
  InterSched sched;
  sched.items = sc.items; sched.ticket = sc.ticket; sched.done = sc.done; sched.error = sc.ticket + 1; sched.total = (unsigned)total; sched.no_wpp = no_wpp;
  sched.wait_ticks = 3000000000ull;  // 30 s of the 100 MHz clock
  const Tables *tb = device_tables();
  void *args[] = { &F, &d_model, &tb, &sched };  // (the kernels' parameters: kvz_inter_kernels.hpp KVZ_ICTU_KERNEL)
  DevTimer &tm = inter_timer();
  if (!tm.e0) { KVZ_HIP_CHECK(hipEventCreate(&tm.e0)); KVZ_HIP_CHECK(hipEventCreate(&tm.e1)); }
  KVZ_HIP_CHECK(hipEventRecord(tm.e0, st));
  KVZ_HIP_CHECK(hipLaunchKernel(inter_build_kernel(unit), dim3((unsigned)n_wg), dim3(KVZ_ICTU_THREADS), args, 0, st));
  KVZ_HIP_CHECK(hipGetLastError());
  KVZ_HIP_CHECK(hipEventRecord(tm.e1, st));
  unsigned flags[2] = { 0, 0 };
  KVZ_HIP_CHECK(hipMemcpyAsync(flags, sc.ticket, sizeof flags, hipMemcpyDeviceToHost, st));
  KVZ_HIP_CHECK(hipStreamSynchronize(st));
  KVZ_HIP_CHECK(hipEventElapsedTime(&inter_kernel_ms(), tm.e0, tm.e1));
  return flags[1] ? -2 : 0;
}
}  // namespace kvz

static int kvz_inter_ctu_pass_run(const uint8_t *src, const uint8_t *ref, const kvz_hip_cu_info *ref_cu, uint8_t *rec, kvz_hip_cu_info *cu, int16_t *coeff, int width,
                                  int height, int n_pictures, const kvz_hip_inter_params *p, const int32_t *tile_xy, int n_references,
                                  const kvz_hip_inter_pictures *pictures, const kvz_hip_scaling_lists *sets, int n_sets, const uint16_t *set_of_picture, int slice_type, const kvz_hip_inter_refs *refs = nullptr);
// pictures == nullptr: p->qp / p->poc for every picture (kvz_hip_dev_inter_ctu_pass[_tiles]); n_sets == 0: no scaling lists (kvz_hip_dev_inter_ctu_pass_pictures)
int kvz_hip_dev_inter_ctu_pass_lists(const uint8_t *src, const uint8_t *ref, const kvz_hip_cu_info *ref_cu, uint8_t *rec, kvz_hip_cu_info *cu, int16_t *coeff, int width,
                                     int height, int n_pictures, const kvz_hip_inter_params *p, const int32_t *tile_xy, int n_references,
                                     const kvz_hip_inter_pictures *pictures, const kvz_hip_scaling_lists *sets, int n_sets, const uint16_t *set_of_picture)
{
  return kvz_inter_ctu_pass_run(src, ref, ref_cu, rec, cu, coeff, width, height, n_pictures, p, tile_xy, n_references, pictures, sets, n_sets, set_of_picture, KVZ_HIP_SLICE_B);
}
// ... of B or of P pictures (kvz_hip_dev.h): KVZ_HIP_SLICE_B is kvz_hip_dev_inter_ctu_pass_pictures
int kvz_hip_dev_inter_ctu_pass_slices(const uint8_t *src, const uint8_t *ref, const kvz_hip_cu_info *ref_cu, uint8_t *rec, kvz_hip_cu_info *cu, int16_t *coeff, int width,
                                      int height, int n_pictures, const kvz_hip_inter_params *p, const int32_t *tile_xy, int n_references,
                                      const kvz_hip_inter_pictures *pictures, int slice_type)
{
  return kvz_inter_ctu_pass_run(src, ref, ref_cu, rec, cu, coeff, width, height, n_pictures, p, tile_xy, n_references, pictures, nullptr, 0, nullptr, slice_type);
}
// ... of P pictures with reference lists (kvz_hip_dev.h): refs == NULL is kvz_hip_dev_inter_ctu_pass_slices; with refs, ref / ref_cu are the pool of refs->n_frames frames
int kvz_hip_dev_inter_ctu_pass_refs(const uint8_t *src, const uint8_t *ref, const kvz_hip_cu_info *ref_cu, uint8_t *rec, kvz_hip_cu_info *cu, int16_t *coeff, int width,
                                    int height, int n_pictures, const kvz_hip_inter_params *p, const int32_t *tile_xy, int n_references,
                                    const kvz_hip_inter_pictures *pictures, int slice_type, const kvz_hip_inter_refs *refs)
{
  return kvz_inter_ctu_pass_run(src, ref, ref_cu, rec, cu, coeff, width, height, n_pictures, p, tile_xy, n_references, pictures, nullptr, 0, nullptr, slice_type, refs);
}
// slice_type: KVZ_HIP_SLICE_B, or -- kvz_hip_dev_inter_ctu_pass_slices / _refs only -- what that entry point was handed; refs: kvz_hip_dev_inter_ctu_pass_refs only
static int kvz_inter_ctu_pass_run(const uint8_t *src, const uint8_t *ref, const kvz_hip_cu_info *ref_cu, uint8_t *rec, kvz_hip_cu_info *cu, int16_t *coeff, int width,
                                  int height, int n_pictures, const kvz_hip_inter_params *p, const int32_t *tile_xy, int n_references,
                                  const kvz_hip_inter_pictures *pictures, const kvz_hip_scaling_lists *sets, int n_sets, const uint16_t *set_of_picture, int slice_type, const kvz_hip_inter_refs *refs)
{
  if (n_pictures <= 0) return 0;
  kvz_hip_inter_params full;
  if (!kvz::inter_params_full(p, &full, "kvz_hip_dev_inter_ctu_pass")) return -1;
  p = &full;  // (a caller from before the me_* members: they are zero)
  if (!kvz::inter_slice_launch_known(p, tile_xy != nullptr, slice_type, "kvz_hip_dev_inter_ctu_pass_slices")) return -1;
  const int refused = kvz::inter_pass_geometry_refused(width, height, n_pictures, p->ref_width, p->ref_height, p->tile_x, p->tile_y);
  if (refused == 1) { fprintf(stderr, "kvz_hip_dev_inter_ctu_pass: bad geometry\n"); return -1; }
  if (pictures && !kvz::inter_pictures_known(pictures, n_pictures, "kvz_hip_dev_inter_ctu_pass_pictures")) return -1;
  if (!kvz::inter_refs_launch_known(refs, n_pictures, pictures != nullptr, pictures ? pictures->poc : nullptr, slice_type, "kvz_hip_dev_inter_ctu_pass_refs")) return -1;
  if (refs && n_references > 0) { fprintf(stderr, "kvz_hip_dev_inter_ctu_pass_refs: n_references %d belongs to tiles of shared frames, which reference lists are not covered with\n", n_references); return -1; }
  if (!pictures && (p->qp < 0 || p->qp > 51)) { fprintf(stderr, "kvz_hip_dev_inter_ctu_pass: picture QP %d outside 0..51\n", p->qp); return -1; }
  if (p->fme_level < 0 || p->fme_level > 4 || p->pu_depth_inter_max < 1 || p->pu_depth_inter_max > 3 || (!pictures && p->poc < 1) || p->fast_residual_cost < 0 || p->fast_residual_cost > 51) { fprintf(stderr, "kvz_hip_dev_inter_ctu_pass: unsupported parameters\n"); return -1; }
  if (refused) {  // the pictures are tiles of a ref_width x ref_height frame
    fprintf(stderr, "kvz_hip_dev_inter_ctu_pass: the %dx%d tile at (%d, %d) does not lie in the %dx%d reference frame, or that frame is beyond what the pass addresses\n", width, height, p->tile_x, p->tile_y, p->ref_width, p->ref_height);
    return -1;
  }
  if (!kvz::scaling_list_sets_known(sets, n_sets, set_of_picture, n_pictures, true /* the pass has no other schedule */, "kvz_hip_dev_inter_ctu_pass_lists")) return -1;
  if (!kvz::inter_me_known(p, (p->ref_width || p->ref_height || tile_xy) ? "tiles" : (n_sets > 0 ? "scaling lists" : nullptr), "kvz_hip_dev_inter_ctu_pass")) return -1;
  const bool lists = n_sets > 0, me = kvz::inter_me_chosen(p), p_slice = slice_type == KVZ_HIP_SLICE_P;  // (P: neither lists -- no entry point hands both over -- nor me)
  hipStream_t st = be().stream;
  const int wc = (width + 63) / 64, hc = (height + 63) / 64, ctus = wc * hc;
  const long total = (long)ctus * n_pictures;
  kvz::InterScratch &sc = kvz::inter_scratch();
  // the kernel's build: with the residual coder's contexts in the LDS context sets only where the picture's coefficients are priced with them (kvz_inter_ctu.hpp)
  // (pictures with QPs of their own: when any of them is; the others run that build with coeff_cabac == 0)
  float fbits[128];
  for (int i = 0; i < 128; i++) fbits[i] = (float)kvz::kEntropyBits[i] / 32768.0f;
  auto model_at_qp = [&](kvz::InterModel *row, int qp) {
    kvz::inter_model_init(row, qp, p->poc, kvz_hip_default_coeff_weights(qp) /* 0 from QP 50 on, where kvz_fast_coeff_cost is never used (rdo.c:311-340) */, fbits, p->mv_constraint, p->sao, p->deblock, p->fme_level, p->pu_depth_inter_max, p->no_wpp, p->fast_residual_cost,
                          width, height, p->ref_width, p->ref_height, p->tile_x, p->tile_y, p->no_tmvp, lists ? 1 : 0, slice_type, refs ? 1 : 0);
    kvz::inter_model_set_me(row, p);
  };
  kvz::InterPictureTable table;
  if (lists) {  // every picture has a record: its rows of the factor table travel with it
    std::vector<int32_t> qp_all, poc_all;
    if (!pictures) { qp_all.assign((size_t)n_pictures, p->qp); poc_all.assign((size_t)n_pictures, p->poc); }
    table = kvz::inter_picture_table_lists(pictures ? pictures->qp : qp_all.data(), pictures ? pictures->poc : poc_all.data(), n_pictures, model_at_qp, sets, n_sets, set_of_picture);
  } else if (refs) table = kvz::inter_picture_table_refs(pictures->qp, pictures->poc, n_pictures, model_at_qp, refs);  // (P, and `pictures` is there: inter_refs_launch_known)
  else if (pictures) table = kvz::inter_picture_table(pictures->qp, pictures->poc, n_pictures, model_at_qp);
  const int build = kvz::inter_build_choose({ (pictures || lists) ? table.any_cabac : kvz::inter_qp_prices_with_cabac(p->qp, p->fast_residual_cost), lists, false, me, p_slice, refs != nullptr });
  if (build == kvz::KVZ_ICTU_BUILD_NONE) { fprintf(stderr, "kvz_hip_dev_inter_ctu_pass: no kernel build for this launch\n"); return -1; }  // (the checks above have refused these, with the reason)
  const int n_wg = kvz::inter_grid(sc, build, total);
  kvz::inter_scratch_reserve(sc, total);
  // the model of the launch, or the table of a launch whose pictures have their own (records, then a row per distinct QP: kvz_inter_host.hpp inter_picture_table)
  kvz::InterModel m;
  if (!pictures && !lists) model_at_qp(&m, p->qp);
  const void *model_image = pictures ? (const void *)table.image.data() : (const void *)&m;
  const size_t model_bytes = lists ? 0 : (pictures ? table.bytes() : sizeof m);
  if (lists) {  // the table with the factor rows has a buffer of its own, which keeps what it holds from call to call
    bool fresh = false;
    if (table.bytes() > sc.lists_bytes) {
      if (sc.lists) KVZ_HIP_CHECK(hipFree(sc.lists));  // (the calling thread's stream is idle: every call ends synchronised)
      sc.lists = nullptr; sc.lists_bytes = 0;
      KVZ_HIP_CHECK(hipMalloc(&sc.lists, table.bytes() + table.bytes() / 8));
      sc.lists_bytes = table.bytes() + table.bytes() / 8;
      fresh = true;
    }
    if (fresh || table.image != sc.h_lists) {
      KVZ_HIP_CHECK(hipMemcpyAsync(sc.lists, table.image.data(), table.bytes(), hipMemcpyHostToDevice, st));
      KVZ_HIP_CHECK(hipStreamSynchronize(st));
      sc.h_lists = table.image;
    }
  }
  if (model_bytes > sc.model_bytes) {
    if (sc.model) KVZ_HIP_CHECK(hipFree(sc.model));
    KVZ_HIP_CHECK(hipMalloc((void **)&sc.model, model_bytes));
    sc.model_bytes = model_bytes;
  }
  std::vector<uint32_t> items;
  kvz::inter_ticket_items(wc, hc, n_pictures, p->no_wpp, items);
  KVZ_HIP_CHECK(hipMemcpyAsync(sc.items, items.data(), (size_t)total * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  if (model_bytes) KVZ_HIP_CHECK(hipMemcpyAsync(sc.model, model_image, model_bytes, hipMemcpyHostToDevice, st));
  KVZ_HIP_CHECK(hipMemsetAsync(sc.done, 0, (size_t)total * sizeof(unsigned), st));
  KVZ_HIP_CHECK(hipMemsetAsync(sc.ticket, 0, 2 * sizeof(unsigned), st));
  KVZ_HIP_CHECK(hipStreamSynchronize(st));  // `items`, `m` and `table` are stack / heap objects of this call
  kvz::InterFrames F;
  F.W = width; F.H = height; F.wc = wc; F.hc = hc; F.frame_px = (long)width * height * 3 / 2; F.cells = (long)(width / 4) * (height / 4);
  F.src = src; F.ref = ref; F.ref_cu = ref_cu; F.rec = rec; F.cu = cu; F.coeff = coeff;
  F.prof = nullptr;
  F.tile_xy = (p->ref_width || p->ref_height) ? tile_xy : nullptr;
  F.ref_count = n_references > 0 ? n_references : 0;
  F.pictures = lists ? (const kvz::InterPicture *)sc.lists : (pictures ? (const kvz::InterPicture *)sc.model : nullptr);
  // the kernel's model argument: what every workgroup loads once per launch -- with a table, picture 0's row (begin_ctu replaces what depends on the picture)
  const kvz::InterModel *d_model = lists ? table.model_of_picture(sc.lists, 0) : (pictures ? table.model_of_picture(sc.model, 0) : (const kvz::InterModel *)sc.model);
#ifdef KVZ_ICTU_PROFILE
  static unsigned long long *d_prof = nullptr;
  if (!d_prof) KVZ_HIP_CHECK(hipMalloc((void **)&d_prof, kvz::IP_COUNT * sizeof(unsigned long long)));
  KVZ_HIP_CHECK(hipMemsetAsync(d_prof, 0, kvz::IP_COUNT * sizeof(unsigned long long), st));
  F.prof = d_prof;
#endif
  const int rc = kvz::inter_launch(sc, build, n_wg, F, d_model, total, p->no_wpp, st);
#ifdef KVZ_ICTU_PROFILE
  {
    unsigned long long hp[kvz::IP_COUNT];
    KVZ_HIP_CHECK(hipMemcpy(hp, d_prof, sizeof hp, hipMemcpyDeviceToHost));
    static const char *names[kvz::IP_COUNT] = { "merge MC+SATD", "early skip", "integer ME", "fractional ME", "candidates", "intra search", "intra recon", "inter quant/recon", "mock+rd cost", "copies", "io", "total search", "winner MC", "context copies", "zero-coeff alternative", "final syntax" };
    for (int i = 0; i < kvz::IP_COUNT; i++) fprintf(stderr, "ictu-profile %-18s %10.3f ms (sum over workgroups) %5.1f %%\n", names[i], hp[i] / 1e5, 100.0 * hp[i] / (double)hp[kvz::IP_TOTAL]);
  }
#endif
  return rc;
}

// Pictures of different sizes in one launch (kvz_inter_joint.hpp): the checks, the ticket list and the table are that header's; the scratch, the grid and the launch
// are what every launch of the pass shares (above)
int kvz_hip_dev_inter_ctu_pass_groups(const kvz_hip_inter_group *groups, int n_groups, const kvz_hip_inter_params *p)
{
  if (!kvz::inter_joint_known(groups, n_groups, p, "kvz_hip_dev_inter_ctu_pass_groups")) return -1;
  kvz_hip_inter_params full;
  kvz::inter_params_full(p, &full, "kvz_hip_dev_inter_ctu_pass_groups");  // (checked above)
  p = &full;
  hipStream_t st = be().stream;
  kvz::InterScratch &sc = kvz::inter_scratch();
  long total = 0;
  for (int i = 0; i < n_groups; i++) total += (long)((groups[i].width + 63) / 64) * ((groups[i].height + 63) / 64) * groups[i].n_pictures;
  kvz::inter_scratch_reserve(sc, total);  // (before the table: the table holds the context scratch's address)
  float fbits[128];
  for (int i = 0; i < 128; i++) fbits[i] = (float)kvz::kEntropyBits[i] / 32768.0f;
  const kvz::InterJointTable table = kvz::inter_joint_table(groups, n_groups, p, sc.ctx, [&](kvz::InterModel *row, int qp) {
    // (no picture size: a row serves every group that has a picture at its QP, and the JOINT builds take ref_w / ref_h from the group record)
    kvz::inter_model_init(row, qp, p->poc, kvz_hip_default_coeff_weights(qp), fbits, p->mv_constraint, p->sao, p->deblock, p->fme_level, p->pu_depth_inter_max, p->no_wpp, p->fast_residual_cost,
                          0, 0, 0, 0, 0, 0, p->no_tmvp, 0);
  });
  const int build = kvz::inter_build_choose({ table.any_cabac, false, true, false, false, false });
  if (build == kvz::KVZ_ICTU_BUILD_NONE) { fprintf(stderr, "kvz_hip_dev_inter_ctu_pass_groups: no kernel build for this launch\n"); return -1; }  // (inter_joint_known has refused these, with the reason)
  const int n_wg = kvz::inter_grid(sc, build, total, n_groups);
  bool fresh = false;
  if (table.bytes() > sc.joint_bytes) {
    if (sc.joint) KVZ_HIP_CHECK(hipFree(sc.joint));  // (the calling thread's stream is idle: every call ends synchronised)
    sc.joint = nullptr; sc.joint_bytes = 0;
    KVZ_HIP_CHECK(hipMalloc(&sc.joint, table.bytes() + table.bytes() / 8));
    sc.joint_bytes = table.bytes() + table.bytes() / 8;
    fresh = true;
  }
  if (fresh || table.image != sc.h_joint) {
    KVZ_HIP_CHECK(hipMemcpyAsync(sc.joint, table.image.data(), table.bytes(), hipMemcpyHostToDevice, st));
    KVZ_HIP_CHECK(hipStreamSynchronize(st));
    sc.h_joint = table.image;
  }
  std::vector<uint32_t> items;
  if (p->no_wpp) kvz::inter_joint_ticket_lists(table.geometry.data(), n_groups, nullptr, &items);
  else kvz::inter_joint_ticket_lists(table.geometry.data(), n_groups, &items, nullptr);
  KVZ_HIP_CHECK(hipMemcpyAsync(sc.items, items.data(), (size_t)total * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  KVZ_HIP_CHECK(hipMemsetAsync(sc.done, 0, (size_t)total * sizeof(unsigned), st));
  KVZ_HIP_CHECK(hipMemsetAsync(sc.ticket, 0, 2 * sizeof(unsigned), st));
  KVZ_HIP_CHECK(hipStreamSynchronize(st));  // `items` is a heap object of this call
  kvz::InterFrames F;
  memset(&F, 0, sizeof F);  // no geometry and no picture buffers: begin_ctu takes them from the drawn picture's group record
  F.pictures = (const kvz::InterPicture *)sc.joint;
  return kvz::inter_launch(sc, build, n_wg, F, table.model_of_picture(sc.joint, 0), total, p->no_wpp, st);
}

float kvz_hip_dev_inter_kernel_ms(void) { return kvz::inter_kernel_ms(); }
void kvz_hip_dev_inter_set_share(int parts) { kvz::inter_share() = parts > 1 ? parts : 1; }
int kvz_hip_dev_inter_slots_per_cu(void)
{
  kvz::runtime_init(-1);
  int fit = 0;
  KVZ_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, kvz::inter_build_kernel(0), KVZ_ICTU_THREADS, 0));
  return fit > 0 ? fit : 8;
}

int kvz_hip_dev_pu_search(const uint8_t *cur, const uint8_t *ref, int width, int height, const kvz_hip_me_pu *pus, int count, int max_pu_size,
                          const kvz_hip_me_params *params, kvz_hip_me_result *out)
{
  if (count <= 0) return 0;
  if (!params || params->fme_level < 0 || params->fme_level > 4) { fprintf(stderr, "kvz_hip_dev_pu_search: fme_level must be 0 .. 4\n"); return -1; }
  const dim3 grid((unsigned)count), block(256);
  const kvz::Tables *tb = kvz::device_tables();
  // PU sizes are mixed within a picture's list: the instantiation is sized for the largest one (pu-depth-inter 1-3: 32)
  if (max_pu_size <= 32) hipLaunchKernelGGL(kvz::dev_pu_search_kernel<32>, grid, block, 0, be().stream, cur, ref, width, height, pus, *params, tb, out);
  else if (max_pu_size <= 64) hipLaunchKernelGGL(kvz::dev_pu_search_kernel<64>, grid, block, 0, be().stream, cur, ref, width, height, pus, *params, tb, out);
  else { fprintf(stderr, "kvz_hip_dev_pu_search: PUs larger than 64 samples do not exist\n"); return -1; }
  KVZ_HIP_CHECK(hipGetLastError());
  return 0;
}

int kvz_hip_dev_inter_pred(const uint8_t *ref0, const uint8_t *ref1, uint8_t *pred, int width, int height, const kvz_hip_mc_pu *pus, int count, int max_pu_size)
{
  if (count <= 0) return 0;
  const dim3 grid((unsigned)count), block(256);
  const kvz::Tables *tb = kvz::device_tables();
  // PUs up to 16x16 with a picture width that is a multiple of 8 (all of kvazaar's): one wavefront per PU
  if (max_pu_size <= 16 && (width & 7) == 0 && !getenv("KVZ_HIP_MC_WORKGROUP_PER_PU"))
    hipLaunchKernelGGL(kvz::dev_inter_pred_wave_kernel, dim3((unsigned)((count + 3) / 4)), block, 0, be().stream, ref0, ref1, pred, width, height, pus, count, tb);
  else if (max_pu_size <= 16) hipLaunchKernelGGL(kvz::dev_inter_pred_kernel<16>, grid, block, 0, be().stream, ref0, ref1, pred, width, height, pus, tb);
  else if (max_pu_size <= 32) hipLaunchKernelGGL(kvz::dev_inter_pred_kernel<32>, grid, block, 0, be().stream, ref0, ref1, pred, width, height, pus, tb);
  else if (max_pu_size <= 64) hipLaunchKernelGGL(kvz::dev_inter_pred_kernel<64>, grid, block, 0, be().stream, ref0, ref1, pred, width, height, pus, tb);
  else { fprintf(stderr, "kvz_hip_dev_inter_pred: PUs larger than 64 samples do not exist\n"); return -1; }
  KVZ_HIP_CHECK(hipGetLastError());
  return 0;
}

void kvz_hip_dev_sao_frames(const uint8_t *in, uint8_t *out, int width, int height, int n_frames, const kvz_hip_sao_params *luma,
                            const kvz_hip_sao_params *chroma)
{
  if (n_frames <= 0) return;
  kvz::launch_sao(be().stream, in, out, width, height, n_frames, nullptr, luma, chroma);
  KVZ_HIP_CHECK(hipGetLastError());
}

int kvz_hip_dev_paste_tiles(uint8_t *frame, int width, int height, const uint8_t *slots, long slot_bytes, const int32_t *tiles /* host: n x (x, y, w, h, slot) */, int n, void *stream)
{
  if (n < 0 || n > 64) { fprintf(stderr, "kvz_hip_dev_paste_tiles: at most 64 tiles per launch\n"); return -1; }
  if (n == 0) return 0;
  kvz::PasteTable tb;
  tb.n = n;
  int hmax = 0;
  for (int i = 0; i < n; i++) {
    tb.x[i] = tiles[5 * i]; tb.y[i] = tiles[5 * i + 1]; tb.w[i] = tiles[5 * i + 2]; tb.h[i] = tiles[5 * i + 3]; tb.slot[i] = tiles[5 * i + 4];
    if (tb.h[i] > hmax) hmax = tb.h[i];
  }
  hipLaunchKernelGGL(kvz::dev_paste_tiles_kernel, dim3(2 * hmax < 512 ? 2 * hmax : 512, n), dim3(256), 0, stream ? (hipStream_t)stream : be().stream, frame, width, height, slots, slot_bytes, tb);
  KVZ_HIP_CHECK(hipGetLastError());
  return 0;
}

void kvz_hip_dev_picture_checksums(const uint8_t *frames, int width, int height, int n_frames, uint32_t *out)
{
  if (n_frames <= 0) return;
  KVZ_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)n_frames * 3 * sizeof(uint32_t), be().stream));
  kvz::launch_checksums(be().stream, frames, width, height, n_frames, out);
  KVZ_HIP_CHECK(hipGetLastError());
}

void kvz_hip_batch_deblock(kvz_hip_batch *b, int qp, int beta_offset_div2, int tc_offset_div2)
{
  kvz::batch_enter(b);
  kvz::deblock_frames_on(b->stream, b->d_rec, b->F.W, b->F.H, b->n_frames, b->d_depth, qp, beta_offset_div2, tc_offset_div2);
}

// kvz_hip_batch_loop_filters (v == nullptr: `model` for every picture) and kvz_hip_batch_loop_filters_models (`model` = the table's first: price table and no_wpp)
// map != nullptr (kvz_hip_batch_loop_filters_ctu_models, with v): deblocking at the QPs of the batch's plane of CU QPs, the SAO decision under every CTU's own lambda
static void kvz_batch_loop_filters_queue(kvz_hip_batch *b, const kvz_hip_intra_cost_model *model, const kvz::ModelTableView *v, int deblock, int beta_offset_div2, int tc_offset_div2, int sao,
                                         const kvz::CtuMapView *map = nullptr)
{
  const uint8_t *cu_qp = map ? b->d_cu_qp : nullptr;
  const kvz::CtuFrames &F = b->F;
  const int n = b->n_frames;
  const int32_t *qps = v ? v->qp_of_picture : nullptr;
  if (!sao) {
    if (deblock) kvz::deblock_frames_on(b->stream, b->d_rec, F.W, F.H, n, b->d_depth, model->qp, beta_offset_div2, tc_offset_div2, 3, nullptr, 0, qps, cu_qp);
    return;
  }
  const size_t pic_bytes = (size_t)F.frame_px * n, lcus = (size_t)F.wc * F.hc * n;
  if (!b->d_ver) {  // first use: the two intermediate pictures and the decision's records
    KVZ_HIP_CHECK(hipMalloc((void **)&b->d_ver, pic_bytes));
    KVZ_HIP_CHECK(hipMalloc((void **)&b->d_dbk, pic_bytes));
    KVZ_HIP_CHECK(hipMalloc((void **)&b->d_sao_stats, lcus * 3 * sizeof(kvz::SaoStats)));
    KVZ_HIP_CHECK(hipMalloc((void **)&b->d_sao_cand, lcus * 3 * sizeof(kvz::SaoCand)));
    KVZ_HIP_CHECK(hipMalloc((void **)&b->d_sao_recs, lcus * 3 * sizeof(kvz::SaoRec)));
    KVZ_HIP_CHECK(hipMalloc((void **)&b->d_sao_merge, lcus));
    KVZ_HIP_CHECK(hipMalloc((void **)&b->d_sao_fbits, 128 * sizeof(float)));
  }
  // R = d_rec (kept), V = d_ver, D = d_dbk
  KVZ_HIP_CHECK(hipMemcpyAsync(b->d_ver, b->d_rec, pic_bytes, hipMemcpyDeviceToDevice, b->stream));
  if (deblock) kvz::deblock_frames_on(b->stream, b->d_ver, F.W, F.H, n, b->d_depth, model->qp, beta_offset_div2, tc_offset_div2, 1, nullptr, 0, qps, cu_qp);
  KVZ_HIP_CHECK(hipMemcpyAsync(b->d_dbk, b->d_ver, pic_bytes, hipMemcpyDeviceToDevice, b->stream));
  if (deblock) kvz::deblock_frames_on(b->stream, b->d_dbk, F.W, F.H, n, b->d_depth, model->qp, beta_offset_div2, tc_offset_div2, 2, nullptr, 0, qps, cu_qp);
  KVZ_HIP_CHECK(hipMemcpyAsync(b->d_sao_fbits, model->entropy_fbits, 128 * sizeof(float), hipMemcpyHostToDevice, b->stream));
  const kvz::SaoGeom g{ F.W, F.H, F.wc, F.hc, F.frame_px };
  hipLaunchKernelGGL(kvz::dev_sao_stats_kernel, dim3((unsigned)(lcus * 3)), dim3(256), 0, b->stream, b->d_src, b->d_rec, b->d_ver, b->d_dbk, g, (kvz::SaoStats *)b->d_sao_stats, (kvz::SaoCand *)b->d_sao_cand);
  if (map) hipLaunchKernelGGL(kvz::dev_sao_chain_kernel_ctu, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, b->stream, (const kvz::SaoStats *)b->d_sao_stats, (const kvz::SaoCand *)b->d_sao_cand, g, n, b->d_sao_fbits, kvz::device_tables(),
                              model->no_wpp, b->d_sao_recs, b->d_sao_merge, v->ctu, map->lambda_of_ctu);
  else hipLaunchKernelGGL(kvz::dev_sao_chain_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, b->stream, (const kvz::SaoStats *)b->d_sao_stats, (const kvz::SaoCand *)b->d_sao_cand, g, n, b->d_sao_fbits, kvz::device_tables(),
                     model->lambda, (int)model->ctx_init[KVZ_HIP_CX_SAO_MERGE], (int)model->ctx_init[KVZ_HIP_CX_SAO_TYPE], model->no_wpp, b->d_sao_recs, b->d_sao_merge, v ? v->ctu : kvz::CtuModelTable());
  // the SAO'd picture becomes the batch's reconstruction (R is not needed any more)
  kvz::launch_sao(b->stream, b->d_dbk, b->d_rec, F.W, F.H, n, b->d_sao_recs, nullptr, nullptr);
  KVZ_HIP_CHECK(hipGetLastError());
}

void kvz_hip_batch_loop_filters(kvz_hip_batch *b, const kvz_hip_intra_cost_model *model, int deblock, int beta_offset_div2, int tc_offset_div2, int sao)
{
  if (!kvz::cost_model_known(model, "kvz_hip_batch_loop_filters")) { b->failed = 1; return; }  // no return value: the batch reports it (kvz_hip_batch_sync -> -1)
  kvz::batch_enter(b);
  kvz_batch_loop_filters_queue(b, model, nullptr, deblock, beta_offset_div2, tc_offset_div2, sao);
}

int kvz_hip_batch_loop_filters_models(kvz_hip_batch *b, const kvz_hip_picture_models *pm, int deblock, int beta_offset_div2, int tc_offset_div2, int sao)
{
  if (!b || !kvz::picture_models_known(pm, b->n_frames, b->sched_ticket != 0, "kvz_hip_batch_loop_filters_models")) return -1;
  kvz::batch_enter(b);
  const kvz::ModelTableView v = kvz::picture_models_stage(b, pm);
  kvz_batch_loop_filters_queue(b, &pm->models[0], &v, deblock, beta_offset_div2, tc_offset_div2, sao);
  return 0;
}

int kvz_hip_batch_loop_filters_ctu_models(kvz_hip_batch *b, const kvz_hip_ctu_models *cm, int deblock, int beta_offset_div2, int tc_offset_div2, int sao)
{
  if (!b || !kvz::ctu_models_known(cm, b->n_frames, b->F.wc * b->F.hc, b->sched_ticket != 0, b->n_list_sets > 0, "kvz_hip_batch_loop_filters_ctu_models")) return -1;
  if (!b->cu_qp_epoch || b->cu_qp_epoch != b->epoch) { fprintf(stderr, "kvz_hip_batch_loop_filters_ctu_models: the batch's last pass was no kvz_hip_intra_frames_ctu_models (the CU QPs come from it)\n"); return -1; }
  kvz::batch_enter(b);
  bool same = false;
  const kvz::CtuMapView map = kvz::ctu_models_stage(b, cm, &same);  // (compares: every CTU's lambda, row and QP)
  if (!same) { fprintf(stderr, "kvz_hip_batch_loop_filters_ctu_models: this is not the map of the batch's last pass (the CU QPs and the lambdas must belong together)\n"); return -1; }
  const kvz::ModelTableView v = kvz::picture_models_stage(b, cm->pictures);
  kvz_batch_loop_filters_queue(b, &cm->pictures->models[0], &v, deblock, beta_offset_div2, tc_offset_div2, sao, &map);
  return 0;
}

int kvz_hip_batch_sao_params(kvz_hip_batch *b, int frame, kvz_hip_sao_params *luma, kvz_hip_sao_params *chroma, uint8_t *merge)
{
  kvz::batch_enter(b);
  const size_t lcus = (size_t)b->F.wc * b->F.hc;
  if (!b->d_sao_recs) { fprintf(stderr, "kvz_hip_batch_sao_params: kvz_hip_batch_loop_filters(..., sao = 1) has not run on this batch\n"); return -1; }
  std::vector<kvz::SaoRec> recs(lcus * 3);
  KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));
  KVZ_HIP_CHECK(hipMemcpy(recs.data(), b->d_sao_recs + (size_t)frame * lcus * 3, lcus * 3 * sizeof(kvz::SaoRec), hipMemcpyDeviceToHost));
  if (merge) KVZ_HIP_CHECK(hipMemcpy(merge, b->d_sao_merge + (size_t)frame * lcus, lcus, hipMemcpyDeviceToHost));
  kvz::sao_recs_unpack(recs.data(), lcus, luma, chroma);
  return kvz::batch_check(b);
}

// The entropy coder in its real mode (kvz_entropy.hpp): the slice data of every picture of the batch, substream by substream, from the device-resident results of the
// CTU pass (and of the loop filters' SAO decision).  Pictures are coded in chunks whose bin records fit a scratch budget (KVZ_HIP_ENTROPY_SCRATCH_MB, default 49152:
// 25 MB per 1080p picture at the default capacity of 12 288 records per CTU); a CTU that produces more records than that makes its chunk run again with the room it needs.
namespace kvz {
// (the initial context states of a B or a P slice in the coder's numbering: kvz_slice_contexts.hpp entropy_slice_contexts)
// scratch of the entropy coder, kept between calls (grow-only; hipMalloc / hipFree per call cost more than a small batch's kernels): one caller at a time
struct EntropyScratch {
  std::mutex lock;
  using Buf = DevBuf;
  Buf bins, nbins, nbits, sizes, ins, offsets, bound_offsets, room, rowctx, scratch, out, not_last;
  hipStream_t side = nullptr;          // stage 2 beside stage 1's second part
  hipEvent_t ev_first = nullptr, ev_rows = nullptr, ev_pre = nullptr;  // ev_pre: everything in front of stage 3 has run (see chain_queued)
  hipEvent_t ev_tail = nullptr;        // behind a call's last kernel, when the call returned with its download in flight
  bool ev_tail_set = false;
  static void *need(Buf &b, size_t bytes)
  {
    if (bytes > b.bytes) {
      if (b.p) KVZ_HIP_CHECK(hipFree(b.p));
      b.bytes = bytes + bytes / 8;
      KVZ_HIP_CHECK(hipMalloc(&b.p, b.bytes));
    }
    return b.p;
  }
};
inline EntropyScratch &entropy_scratch(int device) { static EntropyScratch s[64]; return s[device & 63]; }  // buffers live on the device they were allocated on
}  // namespace kvz
namespace kvz {
// The stages of kvz_entropy.hpp over n_frames pictures, in chunks whose bin records fit the scratch budget.  job(f0, nf): the chunk's inputs (everything of EntropyJob but
// the scratch pointers); not_last: host flags or null.
// own_out: a compaction buffer of the caller's instead of the shared one (grown here); with `defer` the call returns when the LAST chunk's download has been queued on
// `stream` -- the caller synchronises the stream before it reads `out` -- which needs such a buffer: the next call, on another stream, compacts into the shared one at once.
inline long entropy_code_pictures(hipStream_t stream, int device, int n, int wc, int hc, int no_wpp, const uint8_t *not_last, const std::function<EntropyJob(int, int)> &job,
                                  uint8_t *out, size_t capacity, uint32_t *substream_bytes, const std::function<void()> &chain_queued = nullptr,
                                  EntropyScratch::Buf *own_out = nullptr, bool defer = false, const uint32_t *ctu_qp = nullptr)
{
  // ctu_qp (device, [n][ctus]; kvz_hip_batch_entropy_code_ctu_models): the CTUs are quantisation groups -- stage 1 runs as the kernel that codes cu_qp_delta from these words
  EntropyScratch &S = entropy_scratch(device);
  std::lock_guard<std::mutex> guard(S.lock);
  if (S.ev_tail_set) KVZ_HIP_CHECK(hipStreamWaitEvent(stream, S.ev_tail, 0));  // the previous call's last kernels (on its own stream) read scratch this call writes
  static const bool times = getenv("KVZ_HIP_ENTROPY_TIMES") != nullptr;  // developer: host-side phase clock on stderr
  auto t_last = std::chrono::steady_clock::now();
  auto mark = [&](const char *what) { if (!times) return; const auto now = std::chrono::steady_clock::now(); fprintf(stderr, "kvz_hip entropy: %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count()); t_last = now; };
  const int ctus = wc * hc, rows = no_wpp ? 1 : hc;
  size_t budget = 49152;
  if (const char *e = getenv("KVZ_HIP_ENTROPY_SCRATCH_MB")) { const long v = atol(e); if (v > 0) budget = (size_t)v; }
  budget <<= 20;
  uint32_t cap = 12288;
  if (const char *e = getenv("KVZ_HIP_ENTROPY_CAP")) { const long v = atol(e); if (v > 0) cap = ((uint32_t)v + 15u) & ~15u; }
  std::vector<uint32_t> counts, bound_bits, sizes;
  std::vector<unsigned long long> offsets, bound_offsets;
  size_t total = 0;
  long rc = 0;
  for (int f0 = 0; f0 < n && rc == 0;) {
    int nf = (int)(budget / ((size_t)ctus * cap * sizeof(uint32_t)));
    if (nf < 1) nf = 1;
    if (nf > n - f0) nf = n - f0;
    const long items = (long)nf * ctus, streams = (long)nf * rows;
    uint32_t *d_bins = (uint32_t *)S.need(S.bins, (size_t)items * cap * sizeof(uint32_t)), *d_nbins = (uint32_t *)S.need(S.nbins, (size_t)items * sizeof(uint32_t));
    uint32_t *d_nbits = (uint32_t *)S.need(S.nbits, (size_t)items * sizeof(uint32_t)), *d_sizes = (uint32_t *)S.need(S.sizes, (size_t)streams * sizeof(uint32_t));
    unsigned long long *d_offsets = (unsigned long long *)S.need(S.offsets, (size_t)streams * sizeof(unsigned long long));
    unsigned long long *d_bound_offsets = (unsigned long long *)S.need(S.bound_offsets, (size_t)streams * sizeof(unsigned long long));
    uint8_t *d_rowctx = (uint8_t *)S.need(S.rowctx, (size_t)nf * hc * KVZ_ENTROPY_CTXS), *d_out = nullptr, *d_scratch = nullptr;
    uint8_t *d_not_last = not_last ? (uint8_t *)S.need(S.not_last, (size_t)nf) : nullptr;
    if (not_last) KVZ_HIP_CHECK(hipMemcpyAsync(d_not_last, not_last + f0, (size_t)nf, hipMemcpyHostToDevice, stream));
    EntropyJob J = job(f0, nf);
    J.bins = d_bins; J.nbins = d_nbins; J.nbits = d_nbits; J.cap = cap; J.row_ctx = d_rowctx; J.not_last = d_not_last;
    static const bool serial_bins = [] { const char *e = getenv("KVZ_HIP_ENTROPY_BINS"); return e && !strcmp(e, "serial"); }();  // developer: the one-lane-walks-it-all form of stage 1
    // WPP: the row contexts (stage 2: one lane per picture, a long chain) need the bins of the first two CTUs of every row only -- those and stage 2 run on a second
    // stream beside the bins of all the other CTUs
    const bool early_rows = !serial_bins && !no_wpp && wc > 2;
    const uint32_t *words = ctu_qp ? ctu_qp + (size_t)f0 * ctus : nullptr;
    auto bins_part = [&](hipStream_t st, long lanes, int columns) {
      if (words) hipLaunchKernelGGL(dev_entropy_bins_phased_kernel_cuqp, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, st, J, device_tables(), lanes, columns, words);
      else hipLaunchKernelGGL(dev_entropy_bins_phased_kernel, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, st, J, device_tables(), lanes, columns);
    };
    if (serial_bins && !words) hipLaunchKernelGGL(dev_entropy_bins_kernel, dim3((unsigned)((items + 63) / 64)), dim3(64), 0, stream, J, device_tables(), items);
    else if (!early_rows) bins_part(stream, items, 0);
    else {
      const long first = (long)nf * hc * 2, rest = items - first;
      if (!S.side) { KVZ_HIP_CHECK(hipStreamCreateWithFlags(&S.side, hipStreamNonBlocking)); KVZ_HIP_CHECK(hipEventCreateWithFlags(&S.ev_first, hipEventDisableTiming)); KVZ_HIP_CHECK(hipEventCreateWithFlags(&S.ev_rows, hipEventDisableTiming)); }
      KVZ_HIP_CHECK(hipEventRecord(S.ev_first, stream));  // (what the caller queued before -- the pass, the loop filters -- comes first on both streams)
      KVZ_HIP_CHECK(hipStreamWaitEvent(S.side, S.ev_first, 0));
      bins_part(S.side, first, 1);
      hipLaunchKernelGGL(dev_entropy_row_ctx_kernel<8>, dim3((unsigned)((nf + 7) / 8)), dim3(8), 0, S.side, J, device_tables());
      KVZ_HIP_CHECK(hipEventRecord(S.ev_rows, S.side));
      bins_part(stream, rest, 2);
      KVZ_HIP_CHECK(hipStreamWaitEvent(stream, S.ev_rows, 0));  // the counts of every CTU are read next
    }
    counts.resize((size_t)items); bound_bits.resize((size_t)items);
    KVZ_HIP_CHECK(hipMemcpyAsync(counts.data(), d_nbins, (size_t)items * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    KVZ_HIP_CHECK(hipMemcpyAsync(bound_bits.data(), d_nbits, (size_t)items * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    KVZ_HIP_CHECK(hipStreamSynchronize(stream));
    mark("bins + counts down");
    uint32_t most = 0;
    for (uint32_t c : counts) most = c > most ? c : most;
    const bool again = most > cap;
    if (!again) {
      // room per substream: the bound of its CTUs' bits, the coder's flush, and an emulation prevention byte after every two bytes at worst
      bound_offsets.resize((size_t)streams);
      unsigned long long scratch_bytes = 0;
      const long per_stream = no_wpp ? ctus : wc;
      for (long i = 0; i < streams; i++) {
        unsigned long long bits = 0;
        for (long k = 0; k < per_stream; k++) bits += bound_bits[(size_t)(i * per_stream + k)];
        bound_offsets[(size_t)i] = scratch_bytes;
        scratch_bytes += (((bits + 7) / 8 + 16) * 3 / 2 + 15) & ~15ull;
      }
      d_scratch = (uint8_t *)S.need(S.scratch, scratch_bytes ? scratch_bytes : 16);
      mark("host: bounds");
      uint32_t *d_room = (uint32_t *)S.need(S.room, (size_t)streams * sizeof(uint32_t));
      hipLaunchKernelGGL(dev_entropy_stream_room_kernel, dim3((unsigned)((streams + 255) / 256)), dim3(256), 0, stream, d_nbits, streams, per_stream, d_room);
      hipLaunchKernelGGL(dev_entropy_offsets_kernel, dim3(1), dim3(KVZ_ENTROPY_SCAN_THREADS), 0, stream, d_room, streams, d_bound_offsets);  // == bound_offsets, without a copy
      if (chain_queued && f0 + nf >= n) {
        if (!S.ev_pre) KVZ_HIP_CHECK(hipEventCreateWithFlags(&S.ev_pre, hipEventDisableTiming));
        KVZ_HIP_CHECK(hipEventRecord(S.ev_pre, stream));
      }
      static const int lanes = [] { const char *e = getenv("KVZ_HIP_ENTROPY_LANES"); const int v = e ? atoi(e) : 64; return v == 32 || v == 16 || v == 8 ? v : 64; }();
      uint32_t *d_ins = (uint32_t *)S.need(S.ins, (size_t)streams * sizeof(uint32_t));
      if (!early_rows && !no_wpp) hipLaunchKernelGGL(dev_entropy_row_ctx_kernel<8>, dim3((unsigned)((nf + 7) / 8)), dim3(8), 0, stream, J, device_tables());
      {
        const dim3 grid((unsigned)((streams + lanes - 1) / lanes)), block((unsigned)lanes);
        // LDS: a workgroup of this stage takes exactly what a workgroup of the CTU pass takes (unused dynamic LDS on top of its 12 KB).  A pass started beside this stage
        // (kvz_hip_batch_entropy_code_then) is one persistent launch whose workgroups never leave: the 12 KB hole a workgroup of this stage left behind fitted none of them,
        // and every CU that had hosted one ran the rest of the pass with seven workgroups instead of eight
        const unsigned pad = 20480u - (unsigned)(lanes * KVZ_ENTROPY_CTX_STRIDE + 1024);
        if (lanes == 64) hipLaunchKernelGGL(dev_entropy_code_wide_kernel<64>, grid, block, pad, stream, J, device_tables(), streams, d_sizes, d_bound_offsets, d_scratch);
        else if (lanes == 32) hipLaunchKernelGGL(dev_entropy_code_wide_kernel<32>, grid, block, pad, stream, J, device_tables(), streams, d_sizes, d_bound_offsets, d_scratch);
        else if (lanes == 8) hipLaunchKernelGGL(dev_entropy_code_wide_kernel<8>, grid, block, pad, stream, J, device_tables(), streams, d_sizes, d_bound_offsets, d_scratch);
        else hipLaunchKernelGGL(dev_entropy_code_wide_kernel<16>, grid, block, pad, stream, J, device_tables(), streams, d_sizes, d_bound_offsets, d_scratch);
      }
      // from here on the device is nearly idle -- stage 3 is a few hundred wavefronts on their own chains, then a copy --: the caller's moment to queue other work
      // The caller's work is a persistent pass that takes every free workgroup slot the moment it starts: stage 3 must have its slots first (it then runs 39 ms beside
      // the pass; started behind it, it waits 310 ms for the pass to end).  So the pass is queued only when everything in front of stage 3 has run -- stage 3 is then
      // dispatched at once, the pass a launch latency later.
      if (chain_queued && f0 + nf >= n) { KVZ_HIP_CHECK(hipEventSynchronize(S.ev_pre)); chain_queued(); }
      hipLaunchKernelGGL(dev_entropy_escape_count_kernel, dim3((unsigned)streams), dim3(256), 0, stream, d_scratch, d_bound_offsets, d_sizes, d_ins);  // (behind the caller's pass, if it queued one: see kvz_hip_batch_entropy_code_then)
      sizes.resize((size_t)streams);
      KVZ_HIP_CHECK(hipMemcpyAsync(sizes.data(), d_sizes, (size_t)streams * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
      KVZ_HIP_CHECK(hipStreamSynchronize(stream));
      mark("row contexts + coder");
      offsets.resize((size_t)streams);
      unsigned long long chunk_bytes = 0;
      for (long i = 0; i < streams; i++) { offsets[(size_t)i] = chunk_bytes; chunk_bytes += sizes[(size_t)i]; }
      if (total + chunk_bytes > capacity) {
        fprintf(stderr, "kvz_hip_batch_entropy_code: the output buffer is too small (%zu bytes needed so far)\n", (size_t)(total + chunk_bytes));
        rc = -1;
      } else {
        d_out = (uint8_t *)S.need(own_out ? *own_out : S.out, chunk_bytes ? chunk_bytes : 1);
        hipLaunchKernelGGL(dev_entropy_offsets_kernel, dim3(1), dim3(KVZ_ENTROPY_SCAN_THREADS), 0, stream, d_sizes, streams, d_offsets);  // == offsets, without a copy
        hipLaunchKernelGGL(dev_entropy_compact_kernel, dim3((unsigned)streams), dim3(256), 0, stream, d_scratch, d_bound_offsets, d_sizes, d_ins, d_offsets, d_out);
        KVZ_HIP_CHECK(hipGetLastError());
        const bool in_flight = defer && own_out && f0 + nf >= n;
        if (in_flight) {
          if (!S.ev_tail) KVZ_HIP_CHECK(hipEventCreateWithFlags(&S.ev_tail, hipEventDisableTiming));
          KVZ_HIP_CHECK(hipEventRecord(S.ev_tail, stream));
          S.ev_tail_set = true;
        }
        KVZ_HIP_CHECK(hipMemcpyAsync(out + total, d_out, chunk_bytes, hipMemcpyDeviceToHost, stream));
        if (!in_flight) KVZ_HIP_CHECK(hipStreamSynchronize(stream));
        mark("compact + slice data down");
        memcpy(substream_bytes + (size_t)f0 * rows, sizes.data(), (size_t)streams * sizeof(uint32_t));
        total += chunk_bytes;
        f0 += nf;
      }
    }
    if (again) {
      cap = (most + 1023u) & ~1023u;  // this chunk again, with room for its largest CTU
    }
  }
  return rc ? rc : (long)total;
}
}  // namespace kvz

void kvz_hip_batch_entropy_defer_download(kvz_hip_batch *b, int on) { if (b) b->entropy_deferred = on != 0; }

long kvz_hip_batch_entropy_code(kvz_hip_batch *b, const kvz_hip_intra_cost_model *model, int sao, uint8_t *out, size_t capacity, uint32_t *substream_bytes)
{
  return kvz_hip_batch_entropy_code_tiles(b, model, sao, nullptr, out, capacity, substream_bytes);
}
long kvz_hip_batch_entropy_code_tiles(kvz_hip_batch *b, const kvz_hip_intra_cost_model *model, int sao, const uint8_t *not_last, uint8_t *out, size_t capacity,
                                      uint32_t *substream_bytes)
{
  return kvz_hip_batch_entropy_code_then(b, model, sao, not_last, out, capacity, substream_bytes, nullptr, nullptr);
}
// The coder of kvz_hip_batch_entropy_code_then (v == nullptr: `model`'s initial states for every picture) and of kvz_hip_batch_entropy_code_then_models (`model` = the
// table's first: no_wpp, search_nxn).  start_next queues `next`'s pass, once; null when there is none.
static long kvz_batch_entropy_code_queue(kvz_hip_batch *b, const kvz_hip_intra_cost_model *model, const kvz::ModelTableView *v, int sao, const uint8_t *not_last, uint8_t *out,
                                         size_t capacity, uint32_t *substream_bytes, const std::function<void()> &start_next, const uint32_t *ctu_qp = nullptr)
{
  // ctu_qp (kvz_hip_batch_entropy_code_ctu_models, with v): the batch's CTU words -- every CTU codes its cu_qp_delta
  const kvz::CtuFrames &F = b->F;
  const int ctus = F.wc * F.hc;
  if (sao && !b->d_sao_recs) { fprintf(stderr, "kvz_hip_batch_entropy_code: kvz_hip_batch_loop_filters(..., sao = 1) has not run on this batch\n"); return -1; }
  if (model->search_nxn && !b->d_part) { fprintf(stderr, "kvz_hip_batch_entropy_code: the batch has no NxN partition maps\n"); return -1; }
  KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));
  if (kvz::batch_check(b) != 0) return -1;
  const long cells8 = (long)(F.H >> 3) * (F.W >> 3), cells4 = (long)(F.H >> 2) * (F.W >> 2);
  auto job = [&](int f0, int nf) {
    kvz::EntropyJob J;
    memset(&J, 0, sizeof J);
    J.W = F.W; J.H = F.H; J.wc = F.wc; J.hc = F.hc; J.n_frames = nf; J.no_wpp = model->no_wpp;
    J.depth = b->d_depth + f0 * cells8; J.mode = b->d_mode + f0 * cells8;
    J.part = model->search_nxn ? b->d_part + f0 * cells8 : nullptr; J.mode4 = model->search_nxn ? b->d_mode4 + f0 * cells4 : nullptr;
    J.coeff = b->d_coeff + (size_t)f0 * ctus * KVZ_HIP_CTU_COEFFS;
    J.sao = sao ? (const kvz::SaoRec *)b->d_sao_recs + (size_t)f0 * ctus * 3 : nullptr; J.sao_merge = sao ? b->d_sao_merge + (size_t)f0 * ctus : nullptr;
    memcpy(J.ctx_init, model->ctx_init, sizeof model->ctx_init < sizeof J.ctx_init ? sizeof model->ctx_init : sizeof J.ctx_init);
    if (v) { J.ctx_rows = v->ctx_rows; J.model_of_picture = v->ctu.model_of_picture + f0; }
    J.signhide = model->signhide != 0;  // (with a table: every picture by its own model's row)
    return J;
  };
  return kvz::entropy_code_pictures(b->stream, b->device, b->n_frames, F.wc, F.hc, model->no_wpp, not_last, job, out, capacity, substream_bytes,
                                    start_next ? start_next : std::function<void()>(), b->entropy_deferred ? &b->entropy_out : nullptr, b->entropy_deferred != 0, ctu_qp);
}

long kvz_hip_batch_entropy_code_ctu_models(kvz_hip_batch *b, const kvz_hip_ctu_models *cm, int sao, const uint8_t *not_last, uint8_t *out, size_t capacity, uint32_t *substream_bytes)
{
  if (!b || !kvz::ctu_models_known(cm, b->n_frames, b->F.wc * b->F.hc, b->sched_ticket != 0, b->n_list_sets > 0, "kvz_hip_batch_entropy_code_ctu_models")) return -1;
  if (!b->cu_qp_epoch || b->cu_qp_epoch != b->epoch) { fprintf(stderr, "kvz_hip_batch_entropy_code_ctu_models: the batch's last pass was no kvz_hip_intra_frames_ctu_models (the coded deltas come from it)\n"); return -1; }
  if (not_last) { fprintf(stderr, "kvz_hip_batch_entropy_code_ctu_models: tiles are not supported with a model per CTU\n"); return -1; }
  kvz::batch_enter(b);
  bool same = false;
  (void)kvz::ctu_models_stage(b, cm, &same);
  if (!same) { fprintf(stderr, "kvz_hip_batch_entropy_code_ctu_models: this is not the map of the batch's last pass\n"); return -1; }
  const kvz::ModelTableView v = kvz::picture_models_stage(b, cm->pictures);
  return kvz_batch_entropy_code_queue(b, &cm->pictures->models[0], &v, sao, nullptr, out, capacity, substream_bytes, std::function<void()>(), b->d_ctu_qp);
}

long kvz_hip_batch_entropy_code_then(kvz_hip_batch *b, const kvz_hip_intra_cost_model *model, int sao, const uint8_t *not_last, uint8_t *out, size_t capacity,
                                     uint32_t *substream_bytes, kvz_hip_batch *next, const kvz_hip_intra_cost_model *next_model)
{
  if (!b || !kvz::cost_model_known(model, "kvz_hip_batch_entropy_code")) return -1;
  if (next && !kvz::cost_model_known(next_model, "kvz_hip_batch_entropy_code_then (next_model)")) return -3;  // nothing has been queued anywhere
  kvz::batch_enter(b);
  // `next`'s pass is queued exactly once on every path below (the caller synchronises `next` whatever this call returns): by the coder at its quiet moment, or here
  int launched = 0;
  bool started = false;
  // ... and what this call queues behind it on its own stream waits for that pass to end: the coder's last kernels could not run beside a persistent pass anyway (no free
  // workgroup slot), and kernels standing at the head of ANOTHER hardware queue while the pass runs are what one two-batch chain in forty stalled on (DESIGN.md section 8
  // item 8: none with one hardware queue) -- behind an event the queue holds a barrier packet instead of a dispatch
  auto start_next = [&] {
    if (next && !started) {
      started = true;
      launched = kvz_hip_intra_frames(next, next_model);
      kvz::batch_enter(b);
      if (launched > 0) KVZ_HIP_CHECK(hipStreamWaitEvent(b->stream, next->ev1, 0));
    }
  };
  struct StartOnExit { decltype(start_next) &f; ~StartOnExit() { f(); } } start_on_exit{ start_next };
  const long total = kvz_batch_entropy_code_queue(b, model, nullptr, sao, not_last, out, capacity, substream_bytes, next ? std::function<void()>(start_next) : std::function<void()>());
  start_next();  // the coder failed before its last chunk: the pass starts now
  return next && launched < 0 ? -2 : total;
}

long kvz_hip_batch_entropy_code_models(kvz_hip_batch *b, const kvz_hip_picture_models *pm, int sao, const uint8_t *not_last, uint8_t *out, size_t capacity, uint32_t *substream_bytes)
{
  return kvz_hip_batch_entropy_code_then_models(b, pm, sao, not_last, out, capacity, substream_bytes, nullptr, nullptr);
}
long kvz_hip_batch_entropy_code_then_models(kvz_hip_batch *b, const kvz_hip_picture_models *pm, int sao, const uint8_t *not_last, uint8_t *out, size_t capacity,
                                            uint32_t *substream_bytes, kvz_hip_batch *next, const kvz_hip_picture_models *next_pm)
{
  if (!b) return -1;
  if (next && !kvz::picture_models_known(next_pm, next->n_frames, next->sched_ticket != 0, "kvz_hip_batch_entropy_code_then_models (next_models)")) return -3;  // nothing has been queued anywhere
  // as in kvz_hip_batch_entropy_code_then: `next`'s pass is queued exactly once on every path below, the refusal of b's own table included
  int launched = 0;
  bool started = false;
  auto start_next = [&] {
    if (next && !started) {
      started = true;
      launched = kvz_hip_intra_frames_models(next, next_pm);
      kvz::batch_enter(b);
      if (launched > 0) KVZ_HIP_CHECK(hipStreamWaitEvent(b->stream, next->ev1, 0));
    }
  };
  struct StartOnExit { decltype(start_next) &f; ~StartOnExit() { f(); } } start_on_exit{ start_next };
  if (!kvz::picture_models_known(pm, b->n_frames, b->sched_ticket != 0, "kvz_hip_batch_entropy_code_models")) return -1;  // (nothing queued on b)
  kvz::batch_enter(b);
  const kvz::ModelTableView v = kvz::picture_models_stage(b, pm);
  const long total = kvz_batch_entropy_code_queue(b, &pm->models[0], &v, sao, not_last, out, capacity, substream_bytes, next ? std::function<void()>(start_next) : std::function<void()>());
  start_next();
  return next && launched < 0 ? -2 : total;
}

// ... of B pictures: the CU records, levels and (with sao) the SAO decisions of the last kvz_hip_dev_loop_filters_inter as the inter CTU pass / the loop filters left them
long kvz_hip_dev_entropy_code_inter(const kvz_hip_cu_info *cu, const kvz_hip_cu_info *ref_cu, const int16_t *coeff, int width, int height, int n_pictures,
                                    const kvz_hip_inter_params *params, uint8_t *out, size_t capacity, uint32_t *substream_bytes)
{
  return kvz_hip_dev_entropy_code_inter_pictures(cu, ref_cu, coeff, width, height, n_pictures, params, out, capacity, substream_bytes, nullptr);
}
// pictures == nullptr: params->qp / params->poc for every picture (kvz_hip_dev_entropy_code_inter)
long kvz_hip_dev_entropy_code_inter_pictures(const kvz_hip_cu_info *cu, const kvz_hip_cu_info *ref_cu, const int16_t *coeff, int width, int height, int n_pictures,
                                             const kvz_hip_inter_params *params, uint8_t *out, size_t capacity, uint32_t *substream_bytes,
                                             const kvz_hip_inter_pictures *pictures)
{
  return kvz_hip_dev_entropy_code_inter_slices(cu, ref_cu, coeff, width, height, n_pictures, params, out, capacity, substream_bytes, pictures, KVZ_HIP_SLICE_B);
}
static long kvz_entropy_code_inter_run(const kvz_hip_cu_info *cu, const kvz_hip_cu_info *ref_cu, const int16_t *coeff, int width, int height, int n_pictures,
                                       const kvz_hip_inter_params *params, uint8_t *out, size_t capacity, uint32_t *substream_bytes,
                                       const kvz_hip_inter_pictures *pictures, int slice_type, const kvz_hip_inter_refs *refs);
// ... of B or of P pictures (kvz_hip_dev.h): the slice's row of initial states, and no inter_pred_idc in a P slice (kvz_entropy.hpp EntropyJob::p_slice)
long kvz_hip_dev_entropy_code_inter_slices(const kvz_hip_cu_info *cu, const kvz_hip_cu_info *ref_cu, const int16_t *coeff, int width, int height, int n_pictures,
                                           const kvz_hip_inter_params *params, uint8_t *out, size_t capacity, uint32_t *substream_bytes,
                                           const kvz_hip_inter_pictures *pictures, int slice_type)
{
  return kvz_entropy_code_inter_run(cu, ref_cu, coeff, width, height, n_pictures, params, out, capacity, substream_bytes, pictures, slice_type, nullptr);
}
// ... of P pictures with reference lists (kvz_hip_dev.h): refs == NULL is kvz_hip_dev_entropy_code_inter_slices; with refs, ref_cu is the pool's records, ref_idx_l0 is
// coded where a list has more than one entry, and the MVD's predictors are scaled as the pass scaled them (kvz_entropy.hpp EntropyJob::refs)
long kvz_hip_dev_entropy_code_inter_refs(const kvz_hip_cu_info *cu, const kvz_hip_cu_info *ref_cu, const int16_t *coeff, int width, int height, int n_pictures,
                                         const kvz_hip_inter_params *params, uint8_t *out, size_t capacity, uint32_t *substream_bytes,
                                         const kvz_hip_inter_pictures *pictures, int slice_type, const kvz_hip_inter_refs *refs)
{
  return kvz_entropy_code_inter_run(cu, ref_cu, coeff, width, height, n_pictures, params, out, capacity, substream_bytes, pictures, slice_type, refs);
}
// refs: kvz_hip_dev_entropy_code_inter_refs only
static long kvz_entropy_code_inter_run(const kvz_hip_cu_info *cu, const kvz_hip_cu_info *ref_cu, const int16_t *coeff, int width, int height, int n_pictures,
                                       const kvz_hip_inter_params *params, uint8_t *out, size_t capacity, uint32_t *substream_bytes,
                                       const kvz_hip_inter_pictures *pictures, int slice_type, const kvz_hip_inter_refs *refs)
{
  if (n_pictures <= 0) return 0;
  kvz_hip_inter_params full;  // (the coder reads members both known versions of the struct have)
  if (params && !kvz::inter_params_full(params, &full, "kvz_hip_dev_entropy_code_inter")) return -1;
  if (params && !kvz::inter_slice_launch_known(&full, false, slice_type, "kvz_hip_dev_entropy_code_inter_slices")) return -1;
  if (!cu || !ref_cu || !coeff || !params || width <= 0 || height <= 0 || (width & 7) || (height & 7) || (!pictures && (params->qp < 0 || params->qp > 51 || params->poc < 1))) {
    fprintf(stderr, "kvz_hip_dev_entropy_code_inter: bad argument\n");
    return -1;
  }
  if (pictures && !kvz::inter_pictures_known(pictures, n_pictures, "kvz_hip_dev_entropy_code_inter_pictures")) return -1;
  if (!kvz::inter_refs_launch_known(refs, n_pictures, pictures != nullptr, pictures ? pictures->poc : nullptr, slice_type, "kvz_hip_dev_entropy_code_inter_refs")) return -1;
  const int wc = (width + 63) >> 6, hc = (height + 63) >> 6, ctus = wc * hc;
  const long cells4 = (long)(height >> 2) * (width >> 2);
  kvz::LoopScratch &ls = kvz::loop_scratch();
  if (params->sao && (!ls.recs || ls.lcus < (size_t)ctus * n_pictures)) { fprintf(stderr, "kvz_hip_dev_entropy_code_inter: kvz_hip_dev_loop_filters_inter(..., sao = 1) has not run on these pictures\n"); return -1; }
  uint8_t init[KVZ_ENTROPY_CTXS];
  if (!pictures) kvz::entropy_slice_contexts(slice_type, params->qp, init);
  int device = 0;
  KVZ_HIP_CHECK(hipGetDevice(&device));
  // pictures with a QP and a POC of their own: a row of B-slice context states per distinct QP | every picture's POC (0: no temporal predictors) | every picture's row
  // ... and, with reference lists, every picture's list behind them (kvz_inter_refs.hpp InterRefsRecord)
  const uint8_t *d_rows = nullptr; const int32_t *d_poc = nullptr; const uint16_t *d_row_of = nullptr; const kvz::InterRefsRecord *d_refs = nullptr;
  if (pictures) {
    int row_of_qp[52], qp_of_row[52];
    const int n_rows = kvz::inter_qp_rows(pictures->qp, n_pictures, row_of_qp, qp_of_row);
    const size_t at_poc = (size_t)n_rows * KVZ_ENTROPY_CTX_ROW, at_row = at_poc + (size_t)n_pictures * sizeof(int32_t);
    const size_t at_refs = (at_row + (size_t)n_pictures * sizeof(uint16_t) + 3) & ~(size_t)3, bytes = refs ? at_refs + (size_t)n_pictures * sizeof(kvz::InterRefsRecord) : at_row + (size_t)n_pictures * sizeof(uint16_t);
    static_assert(KVZ_ENTROPY_CTX_ROW % 4 == 0 && KVZ_ENTROPY_CTX_ROW >= KVZ_ENTROPY_CTXS, "the POCs behind the rows are 4-byte aligned");
    std::vector<uint8_t> image(bytes, 0);
    for (int r = 0; r < n_rows; r++) kvz::entropy_slice_contexts(slice_type, qp_of_row[r], &image[(size_t)r * KVZ_ENTROPY_CTX_ROW], refs != nullptr);
    for (int i = 0; i < n_pictures; i++) {
      if (refs) ((kvz::InterRefsRecord *)&image[at_refs])[i] = kvz::inter_refs_record(refs, i, pictures->poc[i]);
      ((int32_t *)&image[at_poc])[i] = params->no_tmvp ? 0 : pictures->poc[i];
      ((uint16_t *)&image[at_row])[i] = (uint16_t)row_of_qp[pictures->qp[i]];
    }
    kvz::InterScratch &isc = kvz::inter_scratch();
    if (bytes > isc.entropy_table_bytes) {
      if (isc.entropy_table) KVZ_HIP_CHECK(hipFree(isc.entropy_table));
      KVZ_HIP_CHECK(hipMalloc((void **)&isc.entropy_table, bytes));
      isc.entropy_table_bytes = bytes;
    }
    KVZ_HIP_CHECK(hipMemcpy(isc.entropy_table, image.data(), bytes, hipMemcpyHostToDevice));
    d_rows = isc.entropy_table; d_poc = (const int32_t *)(isc.entropy_table + at_poc); d_row_of = (const uint16_t *)(isc.entropy_table + at_row);
    if (refs) d_refs = (const kvz::InterRefsRecord *)(isc.entropy_table + at_refs);
  }
  auto job = [&](int f0, int nf) {
    kvz::EntropyJob J;
    memset(&J, 0, sizeof J);
    J.W = width; J.H = height; J.wc = wc; J.hc = hc; J.n_frames = nf; J.no_wpp = params->no_wpp;
    J.cu = cu + f0 * cells4; J.ref_cu = refs ? ref_cu /* the pool: a picture's co-located frame is named by its list */ : ref_cu + f0 * cells4; J.poc = params->no_tmvp ? 0 : params->poc;  // (the coder only asks the POC whether temporal predictors exist)
    J.coeff = coeff + (size_t)f0 * ctus * KVZ_HIP_CTU_COEFFS;
    J.sao = params->sao ? ls.recs + (size_t)f0 * ctus * 3 : nullptr; J.sao_merge = params->sao ? ls.merge + (size_t)f0 * ctus : nullptr;
    if (pictures) { J.ctx_rows = d_rows; J.model_of_picture = d_row_of + f0; J.poc_of_picture = d_poc + f0; }
    else memcpy(J.ctx_init, init, sizeof init);
    J.p_slice = slice_type == KVZ_HIP_SLICE_P;
    if (refs) J.refs = d_refs + f0;
    return J;
  };
  return kvz::entropy_code_pictures(be().stream, device, n_pictures, wc, hc, params->no_wpp, nullptr, job, out, capacity, substream_bytes);
}

// ... of I pictures whose results the CALLER put on the device (kvz_hip_dev.h): the I-picture twin of kvz_hip_dev_entropy_code_inter -- kvz_hip_batch_entropy_code's
// coder and kernels on device pointers instead of a batch's buffers, the SAO decisions from host structures
long kvz_hip_dev_entropy_code_intra(const uint8_t *cu_depth, const uint8_t *cu_mode, const uint8_t *cu_part, const uint8_t *cu_mode4, const int16_t *coeff, int width, int height,
                                    int n_pictures, const kvz_hip_intra_cost_model *model, const uint8_t *not_last, const kvz_hip_sao_params *luma,
                                    const kvz_hip_sao_params *chroma, const uint8_t *merge, uint8_t *out, size_t capacity, uint32_t *substream_bytes)
{
  const char *who = "kvz_hip_dev_entropy_code_intra";
  if (!kvz::cost_model_known(model, who)) return -1;
  if (!cu_depth || !cu_mode || !coeff || !out || !substream_bytes) { fprintf(stderr, "%s: a required pointer is NULL\n", who); return -1; }
  if (width <= 0 || height <= 0 || (width & 7) || (height & 7)) { fprintf(stderr, "%s: %d x %d is no picture of positive multiples of 8\n", who, width, height); return -1; }
  if (model->search_nxn && (!cu_part || !cu_mode4)) { fprintf(stderr, "%s: search_nxn without the NxN partition maps\n", who); return -1; }
  const bool sao = luma || chroma || merge;
  if (sao && (!luma || !chroma || !merge)) { fprintf(stderr, "%s: SAO decisions are luma, chroma and merge together, or none of them\n", who); return -1; }
  if (n_pictures <= 0) return 0;
  const int wc = (width + 63) >> 6, hc = (height + 63) >> 6, ctus = wc * hc;
  const long cells8 = (long)(height >> 3) * (width >> 3), cells4 = (long)(height >> 2) * (width >> 2);
  int device = 0;
  KVZ_HIP_CHECK(hipGetDevice(&device));
  kvz::SaoRec *d_recs = nullptr; uint8_t *d_merge = nullptr;
  if (sao) {
    const size_t lcus = (size_t)ctus * n_pictures;
    std::vector<kvz::SaoRec> recs(lcus * 3);
    for (size_t i = 0; i < lcus; i++) { recs[i * 3] = kvz::sao_rec_pack(luma[i], 0); recs[i * 3 + 1] = kvz::sao_rec_pack(chroma[i], 0); recs[i * 3 + 2] = kvz::sao_rec_pack(chroma[i], 1); }
    KVZ_HIP_CHECK(hipMalloc((void **)&d_recs, lcus * 3 * sizeof(kvz::SaoRec)));
    KVZ_HIP_CHECK(hipMalloc((void **)&d_merge, lcus));
    KVZ_HIP_CHECK(hipMemcpy(d_recs, recs.data(), lcus * 3 * sizeof(kvz::SaoRec), hipMemcpyHostToDevice));
    KVZ_HIP_CHECK(hipMemcpy(d_merge, merge, lcus, hipMemcpyHostToDevice));
  }
  auto job = [&](int f0, int nf) {
    kvz::EntropyJob J;
    memset(&J, 0, sizeof J);
    J.W = width; J.H = height; J.wc = wc; J.hc = hc; J.n_frames = nf; J.no_wpp = model->no_wpp;
    J.depth = cu_depth + f0 * cells8; J.mode = cu_mode + f0 * cells8;
    J.part = model->search_nxn ? cu_part + f0 * cells8 : nullptr; J.mode4 = model->search_nxn ? cu_mode4 + f0 * cells4 : nullptr;
    J.coeff = coeff + (size_t)f0 * ctus * KVZ_HIP_CTU_COEFFS;
    J.sao = sao ? d_recs + (size_t)f0 * ctus * 3 : nullptr; J.sao_merge = sao ? d_merge + (size_t)f0 * ctus : nullptr;
    memcpy(J.ctx_init, model->ctx_init, sizeof model->ctx_init < sizeof J.ctx_init ? sizeof model->ctx_init : sizeof J.ctx_init);
    J.signhide = model->signhide != 0;
    return J;
  };
  const long total = kvz::entropy_code_pictures(be().stream, device, n_pictures, wc, hc, model->no_wpp, not_last, job, out, capacity, substream_bytes);  // (returns with its stream drained)
  if (sao) { KVZ_HIP_CHECK(hipFree(d_recs)); KVZ_HIP_CHECK(hipFree(d_merge)); }
  return total;
}

void kvz_hip_dev_picture_md5(const uint8_t *frames, int width, int height, int n_frames, uint8_t *out)
{
  if (n_frames <= 0) return;
  const long n = 3L * n_frames;
  hipLaunchKernelGGL(kvz::dev_md5_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, be().stream, frames, width, height, n, out);
  KVZ_HIP_CHECK(hipGetLastError());
}

int kvz_hip_batch_md5(kvz_hip_batch *b, uint8_t *host_out)
{
  kvz::batch_enter(b);
  const long n = 3L * b->n_frames;
  if (n <= 0) return 0;
  uint8_t *d = nullptr;
  KVZ_HIP_CHECK(hipMallocAsync((void **)&d, (size_t)n * 16, b->stream));
  hipLaunchKernelGGL(kvz::dev_md5_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, b->stream, b->d_rec, b->F.W, b->F.H, n, d);
  KVZ_HIP_CHECK(hipGetLastError());
  KVZ_HIP_CHECK(hipMemcpyAsync(host_out, d, (size_t)n * 16, hipMemcpyDeviceToHost, b->stream));
  KVZ_HIP_CHECK(hipFreeAsync(d, b->stream));
  KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));
  return kvz::batch_check(b);
}

int kvz_hip_batch_checksums(kvz_hip_batch *b, uint32_t *host_out)
{
  kvz::batch_enter(b);
  const int n = b->n_frames;
  if (n <= 0) return 0;
  uint32_t *d = nullptr;
  KVZ_HIP_CHECK(hipMallocAsync((void **)&d, (size_t)n * 3 * sizeof(uint32_t), b->stream));
  KVZ_HIP_CHECK(hipMemsetAsync(d, 0, (size_t)n * 3 * sizeof(uint32_t), b->stream));
  kvz::launch_checksums(b->stream, b->d_rec, b->F.W, b->F.H, n, d);
  KVZ_HIP_CHECK(hipGetLastError());
  KVZ_HIP_CHECK(hipMemcpyAsync(host_out, d, (size_t)n * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
  KVZ_HIP_CHECK(hipFreeAsync(d, b->stream));
  KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));
  return kvz::batch_check(b);
}

int kvz_hip_dev_picture_sse(const uint8_t *a, const uint8_t *b, int width, int height, int n_frames, uint64_t *out)
{
  if (!a || !b || !out || n_frames <= 0 || width <= 0 || height <= 0 || (width & 7) || (height & 7) || (((uintptr_t)a | (uintptr_t)b) & 15) || ((uintptr_t)out & 7)) {
    fprintf(stderr, "kvz_hip_dev_picture_sse: bad argument\n");
    return -1;
  }
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the kernel's 64-bit atomic add");
  KVZ_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)n_frames * 3 * sizeof(uint64_t), be().stream));
  kvz::launch_sse(be().stream, a, b, width, height, n_frames, (unsigned long long *)out);
  KVZ_HIP_CHECK(hipGetLastError());
  return 0;
}

int kvz_hip_batch_sse_async(kvz_hip_batch *b, uint64_t *host_out)
{
  if (!b || !host_out) { fprintf(stderr, "kvz_hip_batch_sse: bad argument\n"); return -1; }
  kvz::batch_enter(b);
  const size_t bytes = (size_t)b->n_frames * 3 * sizeof(uint64_t);
  if (!b->d_sse) KVZ_HIP_CHECK(hipMalloc((void **)&b->d_sse, bytes));
  if (b->up_pending) { KVZ_HIP_CHECK(hipStreamWaitEvent(b->stream, b->ev_up, 0)); b->up_pending = 0; }  // pictures on their way: this call comes after that upload, it sees them
  KVZ_HIP_CHECK(hipMemsetAsync(b->d_sse, 0, bytes, b->stream));
  kvz::launch_sse(b->stream, b->d_src, b->d_rec, b->F.W, b->F.H, b->n_frames, b->d_sse);
  KVZ_HIP_CHECK(hipGetLastError());
  kvz::batch_src_read(b);  // a later kvz_hip_batch_upload_all_async overwrites the source pictures behind this point
  // Pinned memory is written by a kernel, not by the copy engine: in a chain of two batches this point comes right behind the OTHER batch's coder, whose slice data
  // (13 ms per 1 536 1080p pictures) is on its way down then -- a device-to-host copy of these few KB would queue behind it, and this batch's coder behind the copy
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, host_out) == hipSuccess && attr.type == hipMemoryTypeHost && attr.devicePointer) {
    const int n = b->n_frames * 3;
    hipLaunchKernelGGL(kvz::dev_copy_u64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, b->stream, b->d_sse, (unsigned long long *)attr.devicePointer, n);
    KVZ_HIP_CHECK(hipGetLastError());
  } else {
    (void)hipGetLastError();  // (an address the runtime does not know: plain host memory)
    KVZ_HIP_CHECK(hipMemcpyAsync(host_out, b->d_sse, bytes, hipMemcpyDeviceToHost, b->stream));
  }
  return 0;
}

int kvz_hip_batch_sse(kvz_hip_batch *b, uint64_t *host_out)
{
  if (kvz_hip_batch_sse_async(b, host_out) != 0) return -1;
  KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));
  return kvz::batch_check(b);
}

double kvz_hip_psnr(uint64_t sse, long num_pixels)
{
  if (sse == 0) return 999.99;  // encmain.c:107 MAX_PSNR
  return 10.0 * log10(num_pixels * 65025.0 / sse);  // encmain.c:108, 142
}

}  // extern "C"
