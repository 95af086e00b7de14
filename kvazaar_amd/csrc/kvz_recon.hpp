// kvz_recon.hpp -- the integer arithmetic of one sample on its way through intra_recon_tb_leaf (intra.c:561-608) + kvz_quantize_residual (quant-generic.c:198-292),
// each step stated ONCE: the lane decompositions of the intra CTU pass (kvz_ctu.hpp recon_cu8, recon_tus, eval_pu) differ in which samples a lane takes, never in
// what happens to a sample.  Plain functions without state, the same text for the device and the host simulation.  8 bit; flat scaling lists, or -- for the batches
// that were given lists (kvz_hip_batch_set_scaling_lists) -- a forward and an inverse factor per coefficient position (list_index, ListFactor); sign data hiding
// (quant-generic.c:84-176) as a step of its own between quant_level and dequant_level, for the pictures whose model asks for it (sign_hide_group).
#pragma once
#include "kvz_ops.hpp"
#include "kvz_syntax.hpp"

namespace kvz {

// intra.c:262-281: does luma of a 2^log2w block predicted with `mode` read the [1 2 1]-filtered references?  (Chroma never does.)
KVZ_HD bool luma_reads_filtered(int log2w, int mode)
{
  if (mode == 1 || log2w == 2) return false;
  return mode == 0 || imin(iabs(mode - 26), iabs(mode - 10)) > (log2w == 3 ? 7 : (log2w == 4 ? 1 : 0));
}

// What predict_row_segment (kvz_ops.hpp) reads for the LUMA block of a searched 2^log2w CU (log2w 3 or 4), on an image laid out like CtuShared from its `ref` on
// (kMref*: kvz_ops.hpp): the mode's choice of the filtered or unfiltered references, and for the modes 11..25 the row of the extended main references the CU's
// rough search built (Tables::mref_tab).  dc / disp / inv: the block's DC value and the mode's displacement and inverse angle (angular_params).
KVZ_DEV RowRefs searched_luma_refs(const u8 *ref0, int log2w, int mode, int dc, int disp, int inv)
{
  RowRefs rr;
  const unsigned set = luma_reads_filtered(log2w, mode) ? kMrefFiltered : 0u;
  rr.top = ref0 + set; rr.left = ref0 + set + kMrefRefRow;
  rr.ext = mode >= 11 && mode <= 25 ? ref0 + kMrefExtended + kMrefStride * (unsigned)(mode - 11) + kMrefOrg : nullptr;
  rr.dc = dc; rr.disp = disp; rr.inv = inv;
  rr.edges = true;  // intra.c:207-219 intra_post_process_angular, intra-generic.c:210-241: luma below 32 samples
  return rr;
}
// The luma lane roles of a 16x16 CU's reconstruction (kvz_ctu.hpp recon_cu16, stages 1, 3 and 5): lane = row segment of FOUR samples, 64 of them -- row lane >> 2,
// from sample 4 (lane & 3); the segment's elements of a row-major 16x16 buffer start at 4 lane.
struct RowSegment { int py, px0; };
KVZ_HD RowSegment cu16_luma_segment(int lane) { RowSegment g; g.py = lane >> 2; g.px0 = (lane & 3) << 2; return g; }
// Stage 1's luma prediction of recon_cu16 for lane `lane` (0..63): the four samples of its segment
KVZ_DEV void cu16_predict_lane(const u8 *ref0, int mode, int dc, int disp, int inv, int lane, u8 out[4])
{
  const RowSegment g = cu16_luma_segment(lane);
  predict_row_segment<4, true>(4, mode, searched_luma_refs(ref0, 4, mode, dc, disp, inv), g.px0, g.py, out);
}

// One output point of a pass of the N-point transforms (dct-generic.c:559-579).  m(i): the matrix entry that multiplies input i, which is in[at + i] for the
// forward passes (a row) and in[at + i * stride] for the inverse ones (a column).  Forward: the rounded sum wraps to int16 (as the reference's int16 store does);
// inverse: it clips.
template <class Mat> KVZ_DEV i16 fwd_point(int n, Mat m, const i16 *in, int at, int shift)
{
  int a = 0;
  for (int i = 0; i < n; i++) a += m(i) * (int)in[at + i];
  return (i16)((a + (1 << (shift - 1))) >> shift);
}
template <class Mat> KVZ_DEV i16 inv_point(int n, Mat m, const i16 *in, int at, int stride, int shift)
{
  int a = 0;
  for (int k = 0; k < n; k++) a += m(k) * (int)in[k * stride + at];
  return (i16)iclip(-32768, 32767, (a + (1 << (shift - 1))) >> shift);
}

// The same points where the N inputs and the N matrix entries that multiply them are each N / 2 adjacent pairs of int16 (x.w[], m.w[]: Tables::small_pairs holds the
// rows of M and of M^T that way; the inverse passes get their column as a row by reading a buffer that was stored transposed): N / 2 v_dot2_i32_i16.  The sum is the
// exact 32-bit integer in any order (|entry| <= 90, |input| <= 32 768, eight terms).
template <int N, class Row, class MatRow> KVZ_DEV int row_dot(const Row &x, const MatRow &m)
{
  int a = 0;
  for (int i = 0; i < N / 2; i++) a = dot2_i16(x.w[i], m.w[i], a);
  return a;
}
template <int N, class Row, class MatRow> KVZ_DEV i16 fwd_row_point(const Row &x, const MatRow &m, int shift) { return (i16)((row_dot<N>(x, m) + (1 << (shift - 1))) >> shift); }
template <int N, class Row, class MatRow> KVZ_DEV i16 inv_row_point(const Row &x, const MatRow &m, int shift)
{
  return (i16)iclip(-32768, 32767, (row_dot<N>(x, m) + (1 << (shift - 1))) >> shift);
}

// ---- stages 2-5 of the 8x8 CU (kvz_ctu.hpp recon_cu8: one lane per sample e of a 2^L2 block, 8-point luma / 4-point chroma), stated once for the CTU pass, for the
// developer entry point that runs them on blocks without a picture (kvz_dev.hpp kvz_hip_dev_cu8_units) and for its serial host twin (tests/hostsim/hostsim_cu8.cpp).
// t0 / t1: the plane's two scratch buffers of 2^(2 L2) int16, 2^(L2 + 1)-byte aligned.  The lane's inputs are one row of a buffer, read as ONE load; its matrix rows
// (cu8_matrix_rows: row e >> L2 of M for the forward passes, row e & (n - 1) of M^T for the inverse ones, from Tables::small_pairs) stay in registers.  The inverse passes
// read columns, so what they read is stored TRANSPOSED by the stage in front: the caller stores stage 3's dequantised value and cu8_inv_first's result at
// cu8_transposed(e); everything else -- cu8_fwd_first's result, the coefficient, the level, the residual -- belongs to element e.
template <int N> struct alignas(2 * N) Int16Row { u32 w[N / 2]; };
template <int N> KVZ_DEV Int16Row<N> int16_row(const i16 *p)
{
  Int16Row<N> r;
#ifdef KVZ_HOSTSIM
  __builtin_memcpy(&r, p, 2 * N);
#else
  __builtin_memcpy(&r, __builtin_assume_aligned(p, 2 * N), 2 * N);
#endif
  return r;
}
template <int L2> KVZ_HD int cu8_transposed(int e) { return ((e & ((1 << L2) - 1)) << L2) + (e >> L2); }
template <int L2, class MatRow> KVZ_DEV void cu8_matrix_rows(const Tables *tb, int e, MatRow &fwd, MatRow &inv)
{
  constexpr int n = 1 << L2;
  __builtin_memcpy(&fwd, &tb->small_pairs[L2 == 3 ? 1 : 0][0][e >> L2][0], 2 * n);
  __builtin_memcpy(&inv, &tb->small_pairs[L2 == 3 ? 1 : 0][1][e & (n - 1)][0], 2 * n);
}
// forward transform (dct-generic.c:559-568): first pass -> t1[e]; second pass -> the coefficient of element e
template <int L2, class MatRow> KVZ_DEV i16 cu8_fwd_first(const i16 *t0, int e, const MatRow &fwd) { return fwd_row_point<(1 << L2)>(int16_row<(1 << L2)>(t0 + ((e & ((1 << L2) - 1)) << L2)), fwd, L2 - 1); }
template <int L2, class MatRow> KVZ_DEV i16 cu8_fwd_second(const i16 *t1, int e, const MatRow &fwd) { return fwd_row_point<(1 << L2)>(int16_row<(1 << L2)>(t1 + ((e & ((1 << L2) - 1)) << L2)), fwd, L2 + 6); }
// inverse transform (dct-generic.c:570-579) on the transposed intermediates: first pass -> t1[cu8_transposed(e)]; second pass -> the residual of sample e
template <int L2, class MatRow> KVZ_DEV i16 cu8_inv_first(const i16 *t0, int e, const MatRow &inv) { return inv_row_point<(1 << L2)>(int16_row<(1 << L2)>(t0 + ((e >> L2) << L2)), inv, 7); }
template <int L2, class MatRow> KVZ_DEV i16 cu8_inv_second(const i16 *t1, int e, const MatRow &inv) { return inv_row_point<(1 << L2)>(int16_row<(1 << L2)>(t1 + ((e >> L2) << L2)), inv, 12); }

// quant-generic.c:57-81: the level of one coefficient under the forward factor of its position (quant_coeff[n]).  |cf| * q + add < 2^31 for 8-bit flat lists
// (32767 * 26214 + (171 << 18)) and for every list the library accepts: entries >= 13 keep the factor (quant_scale << 4) / entry <= 32263, and
// 32767 * 32263 + (171 << 18) = 1 101 988 445 -- so 32-bit arithmetic is exact.  (A full 32-bit multiply: the factor has 15 bits, the product 30.)
KVZ_HD int quant_level(int cf, const QuantScalars &q, int fwd)
{
  int level = (int)(((u32)iabs(cf) * (u32)fwd + (u32)q.add) >> q.q_bits);
  if (cf < 0) level = -level;
  return iclip(-32768, 32767, level);
}
KVZ_HD int quant_level(int cf, const QuantScalars &q) { return quant_level(cf, q, q.flat_q); }  // flat lists: one factor for the block

// ---- sign data hiding (quant-generic.c:84-176, --signhide): the decoder infers the sign of a coefficient group's first level (lowest scan position) from the parity
// of the group's level sum whenever the first and the last level lie at least four scan positions apart, so the encoder makes the parity fit, by the one change of
// one level by one that costs least.
// quant-generic.c:94 delta_u: what rounding left of the coefficient beyond `level` (the level kvz_quant gave it, before any hiding), in 1/256 of a quantisation
// step: -86 .. 170 in an I slice (add = 171/512 of a step).  |cf| * q and level << q_bits stay below 2^31 (quant_level), their difference lies in [-add, 2^q_bits - add).
KVZ_HD int quant_delta_u(int cf, int level, const QuantScalars &q)
{
  return (int)((u32)iabs(cf) * (u32)q.flat_q - ((u32)iabs(level) << q.q_bits)) >> (q.q_bits - 8);
}
// The rule for ONE coefficient group.  level_at(n) / coeff_at(n): kvz_quant's level and the transform coefficient at scan position n of the group, 0 .. 15.
// first_visited: no group behind this one in scan order holds a level (the reference visits groups last to first: this is the first it meets with a level, and its
// candidate walk starts at the last level instead of position 15).  Returns the change: the scan position whose level moves, -1 for none, and the step, which the
// caller applies with the sign of the COEFFICIENT (sign_hide_apply) -- a zero level leaves zero in the direction its coefficient points.
// The block-level condition of the reference (sum of absolute levels >= 2) needs no statement: a group that takes part holds two levels.  Its +-32767 clamp cannot
// be reached at 8 bit: the largest level is 1638 (QP 0, 4x4 block).
struct SignHideChange { int pos, step; };
template <class LevelAt, class CoeffAt> KVZ_HD SignHideChange sign_hide_group(LevelAt level_at, CoeffAt coeff_at, const QuantScalars &q, bool first_visited)
{
  int first_nz = 16, last_nz = -1, sum = 0;
  for (int n = 0; n < 16; n++) {
    const int l = level_at(n);
    if (l) { if (first_nz == 16) first_nz = n; last_nz = n; }
    sum += l;  // (= the sum from first_nz to last_nz)
  }
  SignHideChange best{ -1, 0 };
  if (last_nz - first_nz < 4) return best;
  const int signbit = level_at(first_nz) > 0 ? 0 : 1;
  if (signbit == (sum & 1)) return best;
  int min_cost = 0x7fffffff;
  for (int n = first_visited ? last_nz : 15; n >= 0; n--) {  // downwards, and only a strictly smaller cost wins: of equal costs the highest position
    const int l = level_at(n), cf = coeff_at(n);
    int cost = 0x7fffffff, step = 0;
    if (l != 0) {
      const int du = quant_delta_u(cf, l, q);
      if (du > 0) { cost = -du; step = 1; }
      else if (n == first_nz && iabs(l) == 1) {}  // would move first_nz
      else { cost = du; step = -1; }
    } else if (n < first_nz && (cf >= 0 ? 0 : 1) != signbit) {}  // would become the first level, with the wrong sign
    else { cost = -quant_delta_u(cf, 0, q); step = 1; }
    if (cost < min_cost) { min_cost = cost; best.pos = n; best.step = step; }
  }
  return best;
}
KVZ_HD int sign_hide_apply(int level, int cf, int step) { return cf >= 0 ? level + step : level - step; }
// Where scan position n of group i (scan order) of a 2^log2w block sits in the row-major block
template <class PtrU8> KVZ_HD int scan_offset(int log2w, int scan_mode, int i, int n, PtrU8 diag8)
{
  const int g = scan_group(log2w, scan_mode, i, diag8), gy = g >> (log2w - 2), gx = g & ((1 << (log2w - 2)) - 1), r = scan_in_group(scan_mode, n);
  return ((gy * 4 + (r >> 2)) << log2w) + gx * 4 + (r & 3);
}
// ... and for a whole block, serially, groups last to first: coeff -> the levels kvz_quant left in `level` (row-major, 2^log2w wide).  What the lanes of the CTU
// pass do a group each (kvz_ctu.hpp hide_signs) and what the tests compare with the per-call oracle.
template <class PtrU8> KVZ_HD void sign_hide_block(const i16 *coeff, i16 *level, int log2w, int scan_mode, const QuantScalars &q, PtrU8 diag8)
{
  bool seen = false;
  for (int i = (1 << (2 * log2w - 4)) - 1; i >= 0; i--) {
    bool any = false;
    for (int n = 0; n < 16; n++) any |= level[scan_offset(log2w, scan_mode, i, n, diag8)] != 0;
    if (!any) continue;
    const SignHideChange ch = sign_hide_group([&](int n) { return (int)level[scan_offset(log2w, scan_mode, i, n, diag8)]; },
                                              [&](int n) { return (int)coeff[scan_offset(log2w, scan_mode, i, n, diag8)]; }, q, !seen);
    seen = true;
    if (ch.pos >= 0) { const int o = scan_offset(log2w, scan_mode, i, ch.pos, diag8); level[o] = (i16)sign_hide_apply(level[o], coeff[o], ch.step); }
  }
}

// quant-generic.c:335-339
KVZ_HD i16 dequant_level(int level, const QuantScalars &q) { return (i16)iclip(-32768, 32767, (level * q.dq_scale + (1 << (q.dq_shift - 1))) >> q.dq_shift); }
// quant-generic.c:309-333: ... under the inverse factor of its position (de_quant_coeff[n] = inv_quant_scale * entry <= 72 * 255; q from quant_scalars with
// scaling_list set: dq_shift = 20 - 14 - transform_shift + 4, dq_qp_per = qp_scaled / 6).  While the shift exceeds qp / 6 the product is rounded and shifted right;
// from qp / 6 == shift on (5 at 4x4, 6 at 8x8, 7 at 16x16, 8 at 32x32) it is clipped, shifted LEFT by the difference and clipped again.  |level * inv| <=
// 32768 * 18360 < 2^30.  With the factor of a flat list (inv_quant_scale * 16) both sides give what the rule above gives.
// (dequant_product: the rule from the product level * inv on, for the caller that multiplies its own way -- the inter pass's 24-bit multiply)
KVZ_HD i16 dequant_product(int prod, const QuantScalars &q)
{
  const int down = q.dq_shift - q.dq_qp_per;
  if (down > 0) return (i16)iclip(-32768, 32767, (prod + (1 << (down - 1))) >> down);
  return (i16)iclip(-32768, 32767, iclip(-32768, 32767, prod) * (1 << -down));
}
KVZ_HD i16 dequant_level(int level, const QuantScalars &q, int inv) { return dequant_product(level * inv, q); }

// ---- per-coefficient scaling lists (scalinglist.c:289-342, 375-391) in compact form: what kvz_scalinglist_set upsamples into a table per block size is indexed
// here the way it is upsampled.  A plane's factors: 16 for 4x4, 64 for 8x8, 64 + the DC term for 16x16 and for 32x32 -- KVZ_LIST_PLANE words, padded to 16 bytes;
// a row = the three planes' factors at one qp % 6.  A word holds the forward factor (quant_level) in its low half and the inverse one (dequant_level) in its high half.
// The all-intra pass keeps rows of the three intra lists; the inter pass rows of all six, intra Y, U, V then inter Y, U, V (KVZ_LIST_ROW_INTER; kvz_scaling_lists.hpp
// scaling_list_rows_inter), and a block of plane c reads list (intra CU ? 0 : 3) + c (quant-generic.c:59, :312).
enum { KVZ_LIST_PLANE = 212, KVZ_LIST_ROW = 3 * KVZ_LIST_PLANE, KVZ_LIST_ROW_INTER = 6 * KVZ_LIST_PLANE };
KVZ_HD int list_plane_of(bool intra_cu, int c) { return (intra_cu ? 0 : 3) + c; }
// where the factors of element e (row-major) of a 2^l2 block are in its plane's part of a row: list entry 8 * (y >> ratio) + (x >> ratio), the DC term for (0, 0)
KVZ_HD int list_index(int l2, int e)
{
  if (l2 == 2) return e;
  const int r = l2 - 3, x = e & ((1 << l2) - 1), y = e >> l2;
  return (l2 == 3 ? 16 : (l2 == 4 ? 80 : 145)) + ((e == 0 && r > 0) ? 64 : 8 * (y >> r) + (x >> r));
}
struct ListFactor { int fwd, inv; };
KVZ_HD ListFactor list_factor(u32 word) { return ListFactor{ (int)(word & 0xffffu), (int)(word >> 16) }; }

// What a level adds to its plane's cost sums: its weight -- `weights`: kvz_hip_intra_cost_model::coeff_weights, four 16-bit prices for |level| = 0, 1, 2, >= 3 -- and
// whether it counts.  word(): both in one, weight | (nonzero << 24), for the stages that reduce one word per plane; such words add up without carrying into the
// count as long as fewer than 256 of them are summed.
struct LevelCost {
  u32 weight, nonzero;
  KVZ_HD u32 word() const { return weight | (nonzero << 24); }
};
KVZ_HD LevelCost level_cost(int level, uint64_t weights)
{
  int a = iabs(level);
  const u32 nz = a != 0;
  if (a > 3) a = 3;
  return LevelCost{ (u32)((weights >> (16 * a)) & 0xffff), nz };
}
// ... with the weights as two 32-bit halves (wavefront-uniform scalars), for the lanes that price eight levels each: a 64-bit shift by a per-lane amount is three
// instructions, the select between two scalars and a 32-bit shift two
KVZ_HD LevelCost level_cost(int level, u32 weights_lo, u32 weights_hi)
{
  int a = iabs(level);
  const u32 nz = a != 0;
  if (a > 3) a = 3;
  return LevelCost{ ((a & 2) ? weights_hi : weights_lo) >> (16 * (a & 1)) & 0xffff, nz };
}

// quant-generic.c:266-277: prediction + residual, clipped to a pixel; search.c:500-505: its squared error against the source
KVZ_HD int recon_sample(int pred, i16 res) { return iclip(0, 255, (int)(i16)(res + pred)); }
KVZ_HD u32 sq_err(int org, int rec) { const int d = org - rec; return (u32)(d * d); }

}  // namespace kvz
