// kvz_recon.hpp -- the integer arithmetic of one sample on its way through intra_recon_tb_leaf (intra.c:561-608) + kvz_quantize_residual (quant-generic.c:198-292),
// each step stated ONCE: the lane decompositions of the intra CTU pass (kvz_ctu.hpp recon_cu8, recon_tus, eval_pu) differ in which samples a lane takes, never in
// what happens to a sample.  Plain functions without state, the same text for the device and the host simulation.  8 bit, flat scaling lists.
#pragma once
#include "kvz_ops.hpp"

namespace kvz {

// intra.c:262-281: does luma of a 2^log2w block predicted with `mode` read the [1 2 1]-filtered references?  (Chroma never does.)
KVZ_HD bool luma_reads_filtered(int log2w, int mode)
{
  if (mode == 1 || log2w == 2) return false;
  return mode == 0 || imin(iabs(mode - 26), iabs(mode - 10)) > (log2w == 3 ? 7 : (log2w == 4 ? 1 : 0));
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

// quant-generic.c:57-81: the level of one coefficient.  |cf| * q + add < 2^31 for 8-bit flat lists (32767 * 26214 + (171 << 18)), so 32-bit arithmetic is exact.
KVZ_HD int quant_level(int cf, const QuantScalars &q)
{
  int level = (int)(((u32)iabs(cf) * (u32)q.flat_q + (u32)q.add) >> q.q_bits);
  if (cf < 0) level = -level;
  return iclip(-32768, 32767, level);
}
// quant-generic.c:335-339
KVZ_HD i16 dequant_level(int level, const QuantScalars &q) { return (i16)iclip(-32768, 32767, (level * q.dq_scale + (1 << (q.dq_shift - 1))) >> q.dq_shift); }

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
