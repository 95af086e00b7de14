// kvz_mfma.hpp -- exact integer matrix products on the matrix cores, shared by the CTU kernel (kvz_ctu.hpp) and the batch
// transform kernels (kvz_dev.hpp).  Device code only.
//
// int8 MFMA with int32 accumulators (v_mfma_i32_32x32x32_i8 / v_mfma_i32_16x16x32_i8): every entry of the transform matrices fits a
// signed byte (|v| <= 90); a 16-bit operand x is split x = 256 h + l into its signed high byte h and its unsigned low byte l, and
// because the instruction wants signed bytes the low part goes in as l - 128 (= l ^ 0x80) with 128 * (sum of the matrix entries it meets)
// preloaded into the accumulator -- together with the rounding constant of the stage.  Everything is exact integer arithmetic
// (|sums| <= 32 * 90 * 128), so results are bit-identical to dct-generic.c whatever the order of summation.
// Splitting four values into byte planes is four v_perm_b32; there are no conversions on either side of the product.
//
// The accumulator layout (lane = column, registers = rows) is the B operand layout of the next product and, read as A, the transposed
// matrix, so a result can feed the next product without leaving registers: the contraction index k only has to sit in the same
// (lane group, byte) slot on both operands, and which k that is is free.  Slot i of a lane carries k = row(lane, i), the row its
// accumulator register i holds; the table operands are stored in that order (Tables::dct_i8, kvz_tables.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "kvz_ops.hpp"

namespace kvz {

typedef int dev_int4 __attribute__((ext_vector_type(4)));
typedef int dev_int16 __attribute__((ext_vector_type(16)));

// byte planes of four 16-bit values (the low halves of v0..v3): lo = (l0 l1 l2 l3) ^ 0x80808080, hi = (h0 h1 h2 h3)
__device__ __forceinline__ void dev_byte_planes(int v0, int v1, int v2, int v3, u32 &lo, u32 &hi)
{
  const u32 t01 = __builtin_amdgcn_perm((u32)v1, (u32)v0, 0x05010400u), t23 = __builtin_amdgcn_perm((u32)v3, (u32)v2, 0x05010400u);
  lo = __builtin_amdgcn_perm(t23, t01, 0x05040100u) ^ 0x80808080u;
  hi = __builtin_amdgcn_perm(t23, t01, 0x07060302u);
}

template <int N> struct DevMma;
template <> struct DevMma<16> {  // v_mfma_i32_16x16x32_i8, the upper half of the k slots left at zero
  static constexpr int NREG = 4;
  static __device__ __forceinline__ int idx(int lane) { return lane & 15; }
  static __device__ __forceinline__ int row(int lane, int r) { return 4 * (lane >> 4) + r; }
  static __device__ __forceinline__ int k0(int lane, int) { return 4 * (lane >> 4); }  // first of the 4 consecutive k of step 0
  static constexpr int STEPS = 1;
};
template <> struct DevMma<32> {  // v_mfma_i32_32x32x32_i8
  static constexpr int NREG = 16;
  static __device__ __forceinline__ int idx(int lane) { return lane & 31; }
  static __device__ __forceinline__ int row(int lane, int r) { return 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3); }
  static __device__ __forceinline__ int k0(int lane, int step) { return 8 * step + 4 * (lane >> 5); }  // slots 4 step .. 4 step + 3
  static constexpr int STEPS = 4;
};

// The 16-point product's operands that do not depend on the block -- this lane's slot of the table and the biases of its accumulator registers --, so that a wavefront
// with several blocks loads them once
struct DevTable16 {
  long tv;       // the table's bytes of this lane's k slots (the upper four slots stay zero: the contraction is over 16)
  int c;         // 128 x the sum of the table row this lane's column meets (register matrix x table)
  dev_int4 s4;   // 128 x the sums of the table rows this lane's four accumulator rows are (table x register matrix)
};
__device__ __forceinline__ DevTable16 dev_table16(const int8_t *tab, const i32 *sums, int lane)
{
  typedef DevMma<16> M;
  DevTable16 t;
  t.tv = (long)(unsigned long long)*reinterpret_cast<const u32 *>(tab + M::idx(lane) * 16 + 4 * (lane >> 4));
  t.c = 128 * sums[M::idx(lane)];
  t.s4 = *reinterpret_cast<const dev_int4 *>(sums + M::row(lane, 0));
  for (int i = 0; i < 4; i++) t.s4[i] *= 128;
  return t;
}
// l, h: the byte planes of the lane's four 16-bit values (dev_byte_planes)
__device__ __forceinline__ void dev_product16_planes(u32 l, u32 h, const DevTable16 &t, bool table_is_a, int add, int *out)
{
  const long lo = (long)(unsigned long long)l, hi = (long)(unsigned long long)h;
  dev_int4 acc = { 0, 0, 0, 0 };
  // ONE accumulator: the high plane's product, times 256 plus the bias, is what the low plane's product adds to
  if (table_is_a) {
    acc = __builtin_amdgcn_mfma_i32_16x16x32_i8(t.tv, hi, acc, 0, 0, 0);
    for (int i = 0; i < 4; i++) acc[i] = acc[i] * 256 + (t.s4[i] + add);
    acc = __builtin_amdgcn_mfma_i32_16x16x32_i8(t.tv, lo, acc, 0, 0, 0);
  } else {
    acc = __builtin_amdgcn_mfma_i32_16x16x32_i8(hi, t.tv, acc, 0, 0, 0);
    for (int i = 0; i < 4; i++) acc[i] = acc[i] * 256 + (t.c + add);
    acc = __builtin_amdgcn_mfma_i32_16x16x32_i8(lo, t.tv, acc, 0, 0, 0);
  }
  for (int r = 0; r < 4; r++) out[r] = acc[r];
}
__device__ __forceinline__ void dev_product16(const int *v, const DevTable16 &t, bool table_is_a, int add, int *out)
{
  u32 l, h;
  dev_byte_planes(v[0], v[1], v[2], v[3], l, h);
  dev_product16_planes(l, h, t, table_is_a, add, out);
}

// out[] = (register matrix v, accumulator layout) x (table) when table_is_a == false, (table) x (register matrix) otherwise, + add.
// tab: the table's rows in slot order (16 or 32 signed bytes per row), sums: the row sums of the table.
template <int N> __device__ __forceinline__ void dev_product(const int *v, const int8_t *tab, const i32 *sums, bool table_is_a, int lane, int add, int *out)
{
  typedef DevMma<N> M;
  if constexpr (N == 32) {
    dev_int4 lo, hi;
    for (int q = 0; q < 4; q++) { u32 l, h; dev_byte_planes(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3], l, h); lo[q] = (int)l; hi[q] = (int)h; }
    const dev_int4 tv = *reinterpret_cast<const dev_int4 *>(tab + M::idx(lane) * 32 + (lane >> 5) * 16);
    // ONE accumulator: the high plane's product first, then 256 x it + the bias as the accumulator the low plane's product adds to -- half the registers of two
    // accumulators and a combining pass (the 32-point products were where the CTU kernel's register allocation spilled)
    dev_int16 acc;
    for (int r = 0; r < 16; r++) acc[r] = 0;
    if (table_is_a) {
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(tv, hi, acc, 0, 0, 0);
      for (int q = 0; q < 4; q++) {
        const dev_int4 s4 = *reinterpret_cast<const dev_int4 *>(sums + M::row(lane, 4 * q));
        for (int i = 0; i < 4; i++) acc[4 * q + i] = acc[4 * q + i] * 256 + (128 * s4[i] + add);
      }
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(tv, lo, acc, 0, 0, 0);
    } else {
      const int c = 128 * sums[M::idx(lane)] + add;
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(hi, tv, acc, 0, 0, 0);
      for (int r = 0; r < 16; r++) acc[r] = acc[r] * 256 + c;
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(lo, tv, acc, 0, 0, 0);
    }
    for (int r = 0; r < 16; r++) out[r] = acc[r];
  } else {
    const DevTable16 t = dev_table16(tab, sums, lane);
    dev_product16(v, t, table_is_a, add, out);
  }
}

// Both passes of a 16- or 32-point DCT / IDCT of one N x N int16 block, chained through registers; `x` and `o` may be the same
// block (every load precedes every store: the stores depend on products that consumed all loads).
//   forward: D0^T = X T^T, K = T D0^T  (dct-generic.c partial_butterfly_*: the intermediate wraps to int16 -- only its two low bytes are used)
//   inverse: U = X^T T,    O = U^T T   (partial_butterfly_inverse_*: both stages clip to int16)
template <int N> __device__ __forceinline__ void mfma_transform_block(const i16 *x, i16 *o, bool inverse, const Tables *tb, int lane)
{
  typedef DevMma<N> M;
  constexpr int L2 = N == 16 ? 4 : 5;
  const int8_t *T = tb->dct_i8[L2 - 4][0], *Tt = tb->dct_i8[L2 - 4][1];
  const i32 *sT = tb->dct_sum[L2 - 4][0], *sTt = tb->dct_sum[L2 - 4][1];
  const int col = M::idx(lane);
  int v[M::NREG], t[M::NREG];
  if (!inverse) {
    for (int st = 0; st < M::STEPS; st++) {  // A operand = rows of X: lane <-> row, four consecutive k per step
      const short4 q = *reinterpret_cast<const short4 *>(x + col * N + M::k0(lane, st));
      v[4 * st] = q.x; v[4 * st + 1] = q.y; v[4 * st + 2] = q.z; v[4 * st + 3] = q.w;
    }
    dev_product<N>(v, T, sT, false, lane, 1 << (L2 - 2), t);
    for (int r = 0; r < M::NREG; r++) v[r] = t[r] >> (L2 - 1);
    dev_product<N>(v, T, sT, true, lane, 1 << (L2 + 5), t);
    for (int r = 0; r < M::NREG; r++) o[M::row(lane, r) * N + col] = (i16)(t[r] >> (L2 + 6));
  } else {
    for (int st = 0; st < M::STEPS; st++)    // A operand = rows of X^T: lane <-> column of X, four consecutive rows per step
      for (int i = 0; i < 4; i++) v[4 * st + i] = x[(M::k0(lane, st) + i) * N + col];
    dev_product<N>(v, Tt, sTt, false, lane, 64, t);
    for (int r = 0; r < M::NREG; r++) v[r] = iclip(-32768, 32767, t[r] >> 7);
    dev_product<N>(v, Tt, sTt, false, lane, 2048, t);   // the accumulator read as A is U^T
    for (int r = 0; r < M::NREG; r++) o[M::row(lane, r) * N + col] = (i16)iclip(-32768, 32767, t[r] >> 12);
  }
}

// NB 16x16 blocks that follow each other in x / o (LDS), one wavefront: the table operands are loaded once and the blocks' chains are independent, so the products of
// one block fill the latency of the others'.  Same arithmetic as mfma_transform_block<16>.
template <int NB> __device__ __forceinline__ void mfma_transform_blocks16(const i16 *x, i16 *o, bool inverse, const Tables *tb, int lane)
{
  typedef DevMma<16> M;
  const int col = M::idx(lane), k0 = M::k0(lane, 0);
  const DevTable16 t = dev_table16(tb->dct_i8[0][inverse ? 1 : 0], tb->dct_sum[0][inverse ? 1 : 0], lane);
  int v[NB][4], w[NB][4];
  const u16 *xu = reinterpret_cast<const u16 *>(x);
#pragma unroll
  for (int b = 0; b < NB; b++) {  // the byte planes come straight out of the 16-bit values as they lie in memory: no sign extension in between
    u32 l, h;
    if (!inverse) {
      const uint2 q = *reinterpret_cast<const uint2 *>(x + b * 256 + col * 16 + k0);
      l = __builtin_amdgcn_perm(q.y, q.x, 0x06040200u) ^ 0x80808080u;
      h = __builtin_amdgcn_perm(q.y, q.x, 0x07050301u);
    } else dev_byte_planes((int)xu[b * 256 + k0 * 16 + col], (int)xu[b * 256 + (k0 + 1) * 16 + col], (int)xu[b * 256 + (k0 + 2) * 16 + col], (int)xu[b * 256 + (k0 + 3) * 16 + col], l, h);
    dev_product16_planes(l, h, t, false, inverse ? 64 : 4, w[b]);
  }
#pragma unroll
  for (int b = 0; b < NB; b++) for (int r = 0; r < 4; r++) v[b][r] = inverse ? iclip(-32768, 32767, w[b][r] >> 7) : w[b][r] >> 3;
#pragma unroll
  for (int b = 0; b < NB; b++) dev_product16(v[b], t, !inverse, inverse ? 2048 : 512, w[b]);
#pragma unroll
  for (int b = 0; b < NB; b++) for (int r = 0; r < 4; r++) o[b * 256 + M::row(lane, r) * 16 + col] = (i16)(inverse ? iclip(-32768, 32767, w[b][r] >> 12) : w[b][r] >> 10);
}

// ---- sum |H8 (P - O) H8| of 32 pairs of 8x8 byte blocks, one wavefront, v_mfma_i32_32x32x32_i8 (the rough search's SATD, kvz_ctu.hpp; kvz_hip_dev_satd8_blocks) ----
// The sum of magnitudes asks for the 64 two-dimensional Walsh functions in any order and with any sign, so the product is W x [P - 128 ; O - 128] with a 64 x 128 matrix
// W = [W64 | -W64] of +-1 bytes (A operand: two tiles of 32 rows, four steps of 32 k) and the samples as they lie in memory, xor 0x80, as B: column = lane & 31 = the
// block, and the lane halves bring rows 0..3 / 4..7 of both blocks, two rows (16 bytes) per step -- P in steps 0 and 1, O in steps 2 and 3.  Which k a (lane half, byte)
// slot is called does not matter: A and B meet slot by slot.  Row m = 32 tile + i of W64 (i = lane & 31) pairs its bits with the sample's
//   bit 5 (tile) <-> step within P / O,   bit 4 <-> lane half,   bit 3 <-> the row within the step,   bits 2..0 <-> the column,
// W64[m][sample] = (-1)^(sum of the paired bits' products): an invertible pairing, so the 64 rows are the 64 Walsh functions, once each.  With the tile bit paired with
// the step, an A fragment is +-(one set of four registers): pos, or neg = -pos, for every (tile, step, P / O).  The accumulators start at kSatdBias > 64 x 255, so
// every output is positive and |coefficient| = |output - bias| is one v_sad_u16 that also adds up.  Exact integers throughout.
struct SatdWalsh { dev_int4 pos, neg; };
constexpr int kSatdBias = 1 << 15;
__device__ __forceinline__ SatdWalsh satd8_walsh(const Tables *tb, int lane)  // this lane's fragment and its negative (Tables::satd_walsh, kvz_ops.hpp satd_walsh_word)
{
  const dev_int4 *row = reinterpret_cast<const dev_int4 *>(tb->satd_walsh[lane]);
  SatdWalsh w;
  w.pos = row[0];
  w.neg = row[1];
  return w;
}
// p, o: the lane's four rows of its column's block (rows 4 (lane >> 5) ..), every byte xor 0x80 (= sample - 128): [0] rows 0 and 1, [1] rows 2 and 3.  Returns the
// block's total on both lanes of the column.
__device__ __forceinline__ u32 satd8_group_mfma(const SatdWalsh &w, const dev_int4 p[2], const dev_int4 o[2])
{
  u32 sums[2] = { 0, 0 };  // two running sums: a v_sad does not wait for the one in front of it
#pragma unroll
  for (int tile = 0; tile < 2; tile++) {  // one tile's sixteen accumulators at a time: the second tile's products start when the first's magnitudes are summed
    dev_int16 t;
#pragma unroll
    for (int r = 0; r < 16; r++) t[r] = kSatdBias;
    t = __builtin_amdgcn_mfma_i32_32x32x32_i8(tile ? w.neg : w.pos, p[1], t, 0, 0, 0);  // (the product that differs first: the tiles share none, and no accumulator outlives its tile)
    t = __builtin_amdgcn_mfma_i32_32x32x32_i8(w.pos, p[0], t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_i32_32x32x32_i8(tile ? w.pos : w.neg, o[1], t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_i32_32x32x32_i8(w.neg, o[0], t, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; r++) sums[r & 1] = __builtin_amdgcn_sad_u16((u32)t[r], (u32)kSatdBias, sums[r & 1]);  // the high halves are zero: v_sad_u16 adds |x - bias| alone
  }
  const u32 sum = sums[0] + sums[1];
  const auto both = __builtin_amdgcn_permlane32_swap(sum, sum, false, false);  // the other half's sum beside this one's, in both halves
  return both[0] + both[1];
}
// Two u16 per register for the row generators (v_pk_mad_u16; bytes widened by v_perm_b32, whose selector value 0x0c reads as a zero byte)
typedef unsigned short U16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ U16x2 u16x2_of(unsigned v) { U16x2 r; __builtin_memcpy(&r, &v, 4); return r; }
__device__ __forceinline__ U16x2 splat16(int v) { U16x2 r; r.x = (unsigned short)v; r.y = (unsigned short)v; return r; }
__device__ __forceinline__ U16x2 widen(unsigned hi, unsigned lo, unsigned sel) { return u16x2_of(__builtin_amdgcn_perm(hi, lo, sel)); }

// ---- the P operand of satd8_group_mfma for a group of 32 (angular mode, block) pairs of an 8x8 / 16x16 CU, from the lane's rows of Tables::satd_rows ----
// e: the lane's four rows ([i >> 1][2 (i & 1)], [.. + 1]: see Tables::satd_rows), ref0: CtuShared::ref with the filtered and extended references and the edge
// bytes behind it.  The row generator is intra-generic.c:125-148 two samples per register with the weights times 8: (32 - f) 8 a + 8 f b + 8 (16 + (128 << 5)) wraps
// mod 2^16, and bits 8..15 of it are the sample xor 0x80, the signed byte the product takes -- no shift, and the packing v_perm_b32 picks the high bytes.  A row of
// modes 10 / 26 that carries intra_post_process_angular's samples gets its first byte xor-ed with the edge byte (satd_edge_byte); every other row's is the zero.
// Nine bytes of the window are used, kSatdWindow are read (Tables::satd_rows keeps the read inside the array's row).
__device__ __forceinline__ void satd_rows_predict(const u8 *ref0, const dev_int4 e[2], dev_int4 p[2])
{
  unsigned rnd_bits = 0x80808080u;  // 8 (16 + (128 << 5)) in both halves
  asm("" : "+v"(rnd_bits));  // opaque, or the compiler pulls the constant out of the multiply-add chain: mul + mad + add where two mads do
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const unsigned w0 = (unsigned)e[i >> 1][2 * (i & 1)], w1 = (unsigned)e[i >> 1][2 * (i & 1) + 1];
    unsigned mw[3];
    static_assert(kSatdWindow == sizeof mw, "the window read");
    __builtin_memcpy(mw, ref0 + (w0 & 0xffff), sizeof mw);
    const unsigned ex = ref0[w0 >> 16];
    const U16x2 wt = u16x2_of(w1), c1 = wt.xx, c0 = splat16(256) - c1, rnd = u16x2_of(rnd_bits);
    // samples k and k + 2 share a register (k = 0, 1, 4, 5): the bytes k, k + 2 and their right neighbours k + 1, k + 3 are six widenings for the eight
    // samples (the odd bytes serve twice, as right neighbours of the even ones and as the samples 1, 3 / 5, 7) where adjacent pairs take eight
    const U16x2 e0 = widen(0, mw[0], 0x0c020c00u), o0 = widen(0, mw[0], 0x0c030c01u), f0 = widen(mw[1], mw[0], 0x0c040c02u);
    const U16x2 e1 = widen(0, mw[1], 0x0c020c00u), o1 = widen(0, mw[1], 0x0c030c01u), f1 = widen(mw[2], mw[1], 0x0c040c02u);
    U16x2 v[4];  // 256 x (the predicted samples xor 0x80) + a remainder below 256: (0, 2), (1, 3), (4, 6), (5, 7)
    v[0] = e0 * c0 + (o0 * c1 + rnd); v[1] = o0 * c0 + (f0 * c1 + rnd);
    v[2] = e1 * c0 + (o1 * c1 + rnd); v[3] = o1 * c0 + (f1 * c1 + rnd);
    unsigned vw[4];
    __builtin_memcpy(vw, v, 16);
    p[i >> 1][2 * (i & 1)] = (int)(__builtin_amdgcn_perm(vw[1], vw[0], 0x07030501u) ^ ex);  // the high bytes of the four u16, in sample order
    p[i >> 1][2 * (i & 1) + 1] = (int)__builtin_amdgcn_perm(vw[3], vw[2], 0x07030501u);
  }
}
// ... and the O operand: the lane's four source rows as they lie in memory, xor 0x80.  cu_org: the CU's origin in the quadrant buffer (vertical modes read their
// rows there; horizontal ones read the transposed block behind ref0).  A lane's rows share the orientation.  Rows are 8-byte aligned.
__device__ __forceinline__ void satd_rows_source(const u8 *ref0, const u8 *cu_org, const dev_int4 e[2], dev_int4 o[2])
{
  const u8 *base = ((unsigned)e[0][1] >> 16 & kSatdSrcVertical) ? cu_org : ref0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const unsigned src = (unsigned)e[i >> 1][2 * (i & 1) + 1] >> 16 & (kSatdSrcVertical - 1);
    unsigned ow[2];
    __builtin_memcpy(ow, __builtin_assume_aligned(base + src, 8), 8);
    o[i >> 1][2 * (i & 1)] = (int)(ow[0] ^ 0x80808080u);
    o[i >> 1][2 * (i & 1) + 1] = (int)(ow[1] ^ 0x80808080u);
  }
}

// out[b] of the blocks 32 group .. 32 group + 31 below count: block b's P at a + 64 b, its O at bsrc + 64 b, row-major
__device__ __forceinline__ void dev_satd8_blocks_wave(const Tables *tb, const u8 *a, const u8 *bsrc, int count, u32 *out, int group, int lane)
{
  const long blk = 32l * group + (lane & 31);
  const bool live = blk < count;
  dev_int4 p[2] = {}, o[2] = {};
  if (live) {
    const dev_int4 *pa = reinterpret_cast<const dev_int4 *>(a + 64 * blk + 32 * (lane >> 5)), *po = reinterpret_cast<const dev_int4 *>(bsrc + 64 * blk + 32 * (lane >> 5));
    p[0] = pa[0]; p[1] = pa[1]; o[0] = po[0]; o[1] = po[1];
  }
#pragma unroll
  for (int q = 0; q < 2; q++) { p[q] ^= (int)0x80808080u; o[q] ^= (int)0x80808080u; }
  const u32 v = satd8_group_mfma(satd8_walsh(tb, lane), p, o);
  if (live && lane < 32) out[blk] = v;
}

}  // namespace kvz
