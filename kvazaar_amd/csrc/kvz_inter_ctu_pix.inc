// kvz_inter_ctu_pix.inc -- part of struct InterCtu (kvz_inter_ctu.hpp): everything that loops over samples, as phases over the workgroup's lanes.
// Pointers into LDS are typed (lu8 / li16 / KVZ_LDS), pictures in HBM are gu8 / gi16: no access of this file is a flat one.

// index arithmetic without integer division (there is none in hardware): powers of two by shifts, the odd window widths (w + 8, w + 7, w + 1 ...) by a
// multiply-shift that is exact for i * d < 2^20
IC_DEV int ilog2i(int w) { return 31 - __builtin_clz((unsigned)w); }
IC_DEV unsigned div_magic(int d) { return d < 32 ? K->div_magic[d] : (1u << 20) / (unsigned)d + 1u; }  // (the divisors are window widths in samples, dwords or runs: small)
IC_DEV int div_by(int i, unsigned magic) { return (int)(umul24((unsigned)i, magic) >> 20); }  // (i < 2^24, magic <= 2^20 + 1)
IC_DEV unsigned long long lds_read64(const lu8 *p) { return *(const KVZ_LDS unsigned long long *)p; }  // 8-byte aligned
IC_DEV u32 lds_read32(const lu8 *p) { return *(const KVZ_LDS u32 *)p; }
IC_DEV void lds_write32(lu8 *p, u32 v) { *(KVZ_LDS u32 *)p = v; }

// ---- sums over a block ----
// The 8x8 Hadamard SATDs (picture-generic.c:252-340: rows, columns, sum of magnitudes, (sum + 2) >> 2) of `ntiles` pairs of 8x8 blocks, EIGHT LANES PER TILE -- the PUs that
// are searched most often are the smallest, and with a lane per tile an 8x8 PU kept one lane busy for six hundred instructions.  Round of eight tiles: lane (slot, r)
// takes row r of its tile's difference through the horizontal butterflies into LDS, lane (slot, c) takes column c through the vertical ones and adds its magnitudes to
// the tile's sum.  src(t, &a, &b): the tile's two blocks (rows 8-byte aligned, strides as / bs); acc(t, satd) runs on one lane per tile.  Scratch: L->g, which is dead
// whenever a SATD runs (the interpolation passes are over; intra prediction does not use it).
// On the device the eight lanes of a tile exchange through DPP, not LDS -- ONE phase, no barrier (the host simulation, whose lanes run one after the other, keeps the
// three-phase form through L->g): lane (slot, r) holds row r of the tile's difference as four packed pairs of 16-bit values (the 8x8 Hadamard of 9-bit differences
// stays below 2^15); butterfly stages commute, so the three vertical stages come first -- partner lanes r ^ 1, r ^ 2 (quad_perm) and r ^ 4 (row_shl / row_shr 4 under
// a bank mask) --, then the horizontal stages k / k + 4 and k / k + 2 on whole registers, and the stage that pairs the halves of a register is folded into the sum of
// magnitudes: |a + b| + |a - b| = 2 max(|a|, |b|).  The tile's sum is then added up over its lanes.
#ifndef KVZ_HOSTSIM
typedef short ic_pk16 __attribute__((ext_vector_type(2)));
IC_DEV ic_pk16 pk_from(int lo, int hi) { ic_pk16 r; r.x = (short)lo; r.y = (short)hi; return r; }
template <int CTRL, int BANKS> IC_DEV ic_pk16 pk_dpp(ic_pk16 old, ic_pk16 v)
{
  int o, x;
  __builtin_memcpy(&o, &old, 4); __builtin_memcpy(&x, &v, 4);
  const int r = __builtin_amdgcn_update_dpp(o, x, CTRL, 0xF, BANKS, false);
  ic_pk16 out;
  __builtin_memcpy(&out, &r, 4);
  return out;
}
IC_DEV u32 pk_absmax2(ic_pk16 a)
{
  const int lo = a.x < 0 ? -(int)a.x : (int)a.x, hi = a.y < 0 ? -(int)a.y : (int)a.y;
  return (u32)(lo > hi ? lo : hi);
}
#endif
template <class Src, class Acc> IC_DEV void satd_tiles(int ntiles, int as, int bs, Src src, Acc acc)
{
#ifndef KVZ_HOSTSIM
  const int tid = threadIdx.x, slot = tid >> 3, r = tid & 7;
  for (int t0 = 0; t0 < ntiles; t0 += KVZ_ICTU_THREADS / 8) {
    const int t = t0 + slot, tt = t < ntiles ? t : ntiles - 1;  // (a lane without a tile repeats the last one: every lane takes part in the exchanges)
    const lu8 *a, *b;
    src(tt, a, b);
    const unsigned long long va = lds_read64(a + r * as), vb = lds_read64(b + r * bs);
    ic_pk16 d[4];
    for (int c = 0; c < 4; c++) d[c] = pk_from((int)((va >> (16 * c)) & 0xff) - (int)((vb >> (16 * c)) & 0xff), (int)((va >> (16 * c + 8)) & 0xff) - (int)((vb >> (16 * c + 8)) & 0xff));
    for (int c = 0; c < 4; c++) {  // rows r and r ^ 1, r ^ 2, r ^ 4: the lane whose bit is clear keeps the sum, the other the difference
      ic_pk16 o = pk_dpp<0xB1 /* quad_perm [1,0,3,2] */, 0xF>(d[c], d[c]);
      d[c] = (r & 1) ? o - d[c] : d[c] + o;
      o = pk_dpp<0x4E /* quad_perm [2,3,0,1] */, 0xF>(d[c], d[c]);
      d[c] = (r & 2) ? o - d[c] : d[c] + o;
      o = pk_dpp<0x104 /* row_shl 4: lane i takes lane i + 4 */, 0x5>(d[c], d[c]);
      o = pk_dpp<0x114 /* row_shr 4: lane i takes lane i - 4 */, 0xA>(o, d[c]);
      d[c] = (r & 4) ? o - d[c] : d[c] + o;
    }
    const ic_pk16 a0 = d[0] + d[2], a1 = d[1] + d[3], a2 = d[0] - d[2], a3 = d[1] - d[3];  // columns k and k + 4
    const ic_pk16 b0 = a0 + a1, b1 = a0 - a1, b2 = a2 + a3, b3 = a2 - a3;                      // columns k and k + 2
    int sum = (int)(2 * (pk_absmax2(b0) + pk_absmax2(b1) + pk_absmax2(b2) + pk_absmax2(b3)));  // columns k and k + 1, folded
    sum += __builtin_amdgcn_update_dpp(0, sum, 0xB1, 0xF, 0xF, false);
    sum += __builtin_amdgcn_update_dpp(0, sum, 0x4E, 0xF, 0xF, false);
    { int o = __builtin_amdgcn_update_dpp(0, sum, 0x104, 0xF, 0x5, false); o = __builtin_amdgcn_update_dpp(o, sum, 0x114, 0xF, 0xA, false); sum += o; }
    if (r == 0 && t < ntiles) acc(t, ((u32)sum + 2) >> 2);
  }
#else
  li16 *sc = (li16 *)L->g;  // eight slots of 8 x 8 values, 72 apart (144 bytes: the slots' columns fall into different banks)
  for (int t0 = 0; t0 < ntiles; t0 += KVZ_ICTU_THREADS / 8) {
    IC_FOR(tid) {
      const int slot = tid >> 3, r = tid & 7, t = t0 + slot;
      if (tid < 8) L->tsum[tid] = 0;
      if (t < ntiles) {
        const lu8 *a, *b;
        src(t, a, b);
        const unsigned long long va = lds_read64(a + r * as), vb = lds_read64(b + r * bs);
        int v[8];
        for (int c = 0; c < 8; c++) v[c] = (int)((va >> (8 * c)) & 0xff) - (int)((vb >> (8 * c)) & 0xff);
        KVZ_HAD8(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
        KVZ_LDS u32 *o = (KVZ_LDS u32 *)(sc + slot * 72 + r * 8);
        for (int c = 0; c < 4; c++) o[c] = ((u32)v[2 * c] & 0xffffu) | ((u32)v[2 * c + 1] << 16);
      }
    }
    IC_SYNC();
    IC_FOR(tid) {
      const int slot = tid >> 3, c = tid & 7, t = t0 + slot;
      if (t < ntiles) {
        const li16 *o = sc + slot * 72 + c;
        int v[8];
        for (int r = 0; r < 8; r++) v[r] = (int)o[r * 8];
        KVZ_HAD8(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
        u32 s = 0;
        for (int r = 0; r < 8; r++) s += (u32)iabs(v[r]);
        IC_LDS_ADD(&L->tsum[slot], s);
      }
    }
    IC_SYNC();
    IC_FOR(tid) {
      const int slot = tid >> 3, t = t0 + slot;
      if ((tid & 7) == 0 && t < ntiles) acc(t, (L->tsum[slot] + 2) >> 2);
    }
    IC_SYNC();
  }
#endif
}
// kvz_satd_any_size for a w x w block (multiples of 8): 8x8 Hadamard tiles, (sum + 2) >> 2 each (picture-generic.c:252-340, strategies-picture.h:75-113)
IC_FN u32 satd_block(const lu8 *a, int as, const lu8 *b, int bs, int w)
{
  const int tw = w >> 3, l2t = ilog2i(tw);
  u32 part = 0;
  satd_tiles(tw * tw, as, bs,
             [=](int t, const lu8 *&pa, const lu8 *&pb) { const int ty = t >> l2t, tx = t & (tw - 1); pa = a + ty * 8 * as + tx * 8; pb = b + ty * 8 * bs + tx * 8; },
             [&](int, u32 v) { part += v; });
  return lanes_sum(part);
}
// the three kvz_pixels_calc_ssd (picture-generic.c:536-551) of a CU (luma w x w at (xl, yl), chroma cw x cw) between the source and level lv's reconstruction in one
// phase, four samples per step: L->ssd[0] luma, L->ssd[1] U + V
IC_FN void ssd_cu(int lv, int xl, int yl, int w, int cw)
{
  u32 pl = 0, pc = 0;
  const int l2 = ilog2i(w), l2c = ilog2i(cw);
  const PView a = orgv(0, xl, yl), b = lvl(lv, 0, xl, yl), au = orgv(1, xl, yl), bu = lvl(lv, 1, xl, yl), av = orgv(2, xl, yl), bv = lvl(lv, 2, xl, yl);
  IC_FOR(tid) {
    for (int i = tid; i < (w * w) >> 2; i += KVZ_ICTU_THREADS) {
      const int y = i >> (l2 - 2), x4 = (i & ((w >> 2) - 1)) << 2;
      const u32 va = lds_read32(a.p + y * a.s + x4), vb = lds_read32(b.p + y * b.s + x4);
      for (int k = 0; k < 4; k++) { const int d = (int)((va >> (8 * k)) & 0xff) - (int)((vb >> (8 * k)) & 0xff); pl += (u32)(d * d); }
    }
    for (int i = tid; i < (cw * cw) >> 1; i += KVZ_ICTU_THREADS) {
      const int c = i >> (2 * l2c - 2), j = i & (((cw * cw) >> 2) - 1), y = j >> (l2c - 2), x4 = (j & ((cw >> 2) - 1)) << 2;
      const u32 va = c == 0 ? lds_read32(au.p + y * au.s + x4) : lds_read32(av.p + y * av.s + x4), vb = c == 0 ? lds_read32(bu.p + y * bu.s + x4) : lds_read32(bv.p + y * bv.s + x4);
      for (int k = 0; k < 4; k++) { const int d = (int)((va >> (8 * k)) & 0xff) - (int)((vb >> (8 * k)) & 0xff); pc += (u32)(d * d); }
    }
  }
  L->ssd[0] = lanes_sum(pl);
  L->ssd[1] = lanes_sum(pc);
}

// ---- the source samples (init_lcu_t, search.c:1160-1180), one 32x32 quadrant of the CTU at a time: zero outside the picture ----
IC_FN void load_org_quadrant(int qx, int qy)  // luma position of the quadrant in the picture
{
  IC_FOR(tid) {
    for (int i = tid; i < 384; i += KVZ_ICTU_THREADS) {  // four samples each: picture sizes are multiples of 8, a dword lies inside or outside
      const int c = i < 256 ? 0 : (i < 320 ? 1 : 2), j = i - (c == 0 ? 0 : (c == 1 ? 256 : 320)), l2 = c ? 2 : 3, y = j >> l2, x4 = (j & ((1 << l2) - 1)) << 2;
      const int px = (qx >> (c ? 1 : 0)) + x4, py = (qy >> (c ? 1 : 0)) + y, pw = F.W >> (c ? 1 : 0), ph = F.H >> (c ? 1 : 0);
      const u32 v = (px < pw && py < ph) ? *(const KVZ_GLB u32 *)(srcp(c) + (py * pw + px)) : 0u;
      ((KVZ_LDS u32 *)L->orgq)[i] = v;
    }
  }
  IC_SYNC();
}
IC_DEV CuInfo zero_cu()
{
  CuInfo z;
  z.type = 0; z.depth = 0; z.mode = 0; z.tr_depth = 0; z.cbf = 0; z.skipped = 0; z.merged = 0; z.merge_idx = 0; z.mv_dir = 0;
  z.mv_ref[0] = z.mv_ref[1] = 0; z.mv_cand[0] = z.mv_cand[1] = 0; z.mv[0][0] = z.mv[0][1] = z.mv[1][0] = z.mv[1][1] = 0;
  return z;
}
// FILL(*lcu, 0) of the CU records (search.c:1160): the decided picture's
IC_FN void clear_cu_records()
{
  IC_FOR(tid) { for (int i = tid; i < (int)(sizeof L->Dcu / 4); i += KVZ_ICTU_THREADS) ((KVZ_LDS u32 *)L->Dcu)[i] = 0; }
  IC_SYNC();
}

// The depth-`depth` CU at (xl, yl), evaluated in level `depth`, is final as far as its own subtree goes (it was not split, or the split lost): the work-tree copies
// of search.c:943-1063 (copy_cu_info / copy_cu_pixels down to every deeper level) = candidate -> decided picture.  Records: the CU's first 4x4 unit carries `cu` (it
// IS the reference's cur_cu); the other units of an inter CU are copies of it (lcu_fill_cu_info, search.c:137-159), those of an intra CU carry type, depth, mode and
// tr_depth and are otherwise still zero -- one record per 8x8 here, so the first 8x8 holds `cu` and the rest the unit record.  Levels: a candidate whose levels wait in
// the workgroup's scratch (depth 1, 2) and that has any go to the output block -- a CU without coded coefficients leaves nothing to read there.
IC_FN void commit_down(int depth, int xl, int yl)
{
  const CuInfo cu = L->cur_cu[depth];
  const int w = 64 >> depth, l2 = ilog2i(w), lb = l2 - 3, blocks = 1 << (2 * lb);
  // the record as eleven half-words in registers, and the unit record's (an intra CU's other cells keep type, depth, mode, tr_depth and zeros): chosen word by word --
  // a choice between two records, `i == 0 ? cu : unit`, goes through the stack
  union Rec { CuInfo c; uint16_t h[11]; };
  Rec rc, ru;
  rc.c = cu;
  ru.c = cu;
  if (cu.type == 1) { ru.c = zero_cu(); ru.c.type = cu.type; ru.c.depth = cu.depth; ru.c.mode = cu.mode; ru.c.tr_depth = cu.tr_depth; }
  const PView sy = lvl(depth, 0, xl, yl), su = lvl(depth, 1, xl, yl), sv = lvl(depth, 2, xl, yl);
  gu8 *dy = recp(0) + ((cy + yl) * F.W + cx + xl), *du = recp(1) + (((cy + yl) >> 1) * (F.W >> 1) + ((cx + xl) >> 1)), *dv = recp(2) + (((cy + yl) >> 1) * (F.W >> 1) + ((cx + xl) >> 1));
  const bool levels = depth < 3 && cu.type != 0 && !cu.skipped && cbf_any(cu.cbf, depth);
  IC_FOR(tid) {
    for (int i = tid; i < blocks; i += KVZ_ICTU_THREADS) { const int yy = i >> lb, xx = i & ((1 << lb) - 1); uint16_t *cell = (uint16_t *)dcell(xl + 8 * xx, yl + 8 * yy); for (int k = 0; k < 11; k++) cell[k] = i == 0 ? rc.h[k] : ru.h[k]; }
    for (int i = tid; i < (w * w) >> 2; i += KVZ_ICTU_THREADS) { const int yy = i >> (l2 - 2), x4 = (i & ((w >> 2) - 1)) << 2; *(KVZ_GLB u32 *)(dy + (yy * F.W + x4)) = lds_read32(sy.p + yy * sy.s + x4); }
    const int cw = w >> 1, l2c = l2 - 1;
    for (int i = tid; i < (cw * cw) >> 1; i += KVZ_ICTU_THREADS) {  // U and V, four samples each
      const int c = i >> (2 * l2c - 2), j = i & (((cw * cw) >> 2) - 1), yy = j >> (l2c - 2), x4 = (j & ((cw >> 2) - 1)) << 2;
      if (c == 0) *(KVZ_GLB u32 *)(du + (yy * (F.W >> 1) + x4)) = lds_read32(su.p + yy * su.s + x4); else *(KVZ_GLB u32 *)(dv + (yy * (F.W >> 1) + x4)) = lds_read32(sv.p + yy * sv.s + x4);
    }
    if (levels) {
      const KVZ_GLB u32 *fy = (const KVZ_GLB u32 *)coef(depth, 0, xl, yl), *fu = (const KVZ_GLB u32 *)coef(depth, 1, xl, yl), *fv = (const KVZ_GLB u32 *)coef(depth, 2, xl, yl);
      KVZ_GLB u32 *ty = (KVZ_GLB u32 *)coef(3, 0, xl, yl), *tu = (KVZ_GLB u32 *)coef(3, 1, xl, yl), *tv = (KVZ_GLB u32 *)coef(3, 2, xl, yl);
      for (int i = tid; i < (w * w) >> 1; i += KVZ_ICTU_THREADS) ty[i] = fy[i];
      for (int i = tid; i < (cw * cw) >> 1; i += KVZ_ICTU_THREADS) { tu[i] = fu[i]; tv[i] = fv[i]; }
    }
  }
  IC_SYNC();
}

// cu_zero_coeff_cost's side copy of the depth-lv CU's samples (search.c:222, 533-547): park = candidate -> parking place, else back
IC_FN void copy_cu_samples(int lv, int xl, int yl, int w, bool park)
{
  const int l2 = ilog2i(w), cw = w >> 1, l2c = l2 - 1;
  const PView f0 = park ? lvl(lv, 0, xl, yl) : parked(lv, 0, xl, yl), t0 = park ? parked(lv, 0, xl, yl) : lvl(lv, 0, xl, yl);
  const PView f1 = park ? lvl(lv, 1, xl, yl) : parked(lv, 1, xl, yl), t1 = park ? parked(lv, 1, xl, yl) : lvl(lv, 1, xl, yl);
  const PView f2 = park ? lvl(lv, 2, xl, yl) : parked(lv, 2, xl, yl), t2 = park ? parked(lv, 2, xl, yl) : lvl(lv, 2, xl, yl);
  IC_FOR(tid) {
    for (int i = tid; i < (w * w) >> 2; i += KVZ_ICTU_THREADS) { const int yy = i >> (l2 - 2), x4 = (i & ((w >> 2) - 1)) << 2; lds_write32(t0.p + yy * t0.s + x4, lds_read32(f0.p + yy * f0.s + x4)); }
    for (int i = tid; i < (cw * cw) >> 1; i += KVZ_ICTU_THREADS) {
      const int c = i >> (2 * l2c - 2), j = i & (((cw * cw) >> 2) - 1), yy = j >> (l2c - 2), x4 = (j & ((cw >> 2) - 1)) << 2;
      if (c == 0) lds_write32(t1.p + yy * t1.s + x4, lds_read32(f1.p + yy * f1.s + x4)); else lds_write32(t2.p + yy * t2.s + x4, lds_read32(f2.p + yy * f2.s + x4));
    }
  }
  IC_SYNC();
}

// a w x w luma block from one view to another, four samples per step
IC_FN void copy_luma(const PView f, const PView t, int w)
{
  const int l2 = ilog2i(w);
  IC_FOR(tid) { for (int i = tid; i < (w * w) >> 2; i += KVZ_ICTU_THREADS) { const int yy = i >> (l2 - 2), x4 = (i & ((w >> 2) - 1)) << 2; lds_write32(t.p + yy * t.s + x4, lds_read32(f.p + yy * f.s + x4)); } }
  IC_SYNC();
}

// ---- motion estimation (oracle: mv_allowed .. search_frac); the PU is L->pu ----
IC_DEV bool mv_allowed(int x, int y)
{
  if (!M->mv_constraint) return true;
  const PuSearch &pu = L->pu;
  const bool frac_luma = (x % 4 != 0) || (y % 4 != 0), frac_chroma = (x % 8 != 0) || (y % 8 != 0);
  int margin = frac_luma ? 4 : (frac_chroma ? 2 : 0);
  if (M->sao) margin += 10; else if (M->deblock) margin += 8;
  const int lx = ((pu.x + pu.w + margin) * 4 + x) / 256 - pu.x / 64, ly = ((pu.y + pu.w + margin) * 4 + y) / 256 - pu.y / 64;
  return !(ly > 1) && !(lx + ly > 2);
}
IC_DEV unsigned golomb_bits(unsigned s)
{
  unsigned bins = 0;
  if (s >= 1u << 8) { bins += 16; s >>= 8; }
  if (s >= 1u << 4) { bins += 8; s >>= 4; }
  if (s >= 1u << 2) { bins += 4; s >>= 2; }
  if (s >= 1u << 1) bins += 2;
  return bins;
}
IC_DEV int mvd_coding_bits(int dx, int dy)
{
  const unsigned ax = (unsigned)iabs(dx), ay = (unsigned)iabs(dy);
  return (int)(4 + (ax == 1) + (ay == 1) + golomb_bits(ax) + golomb_bits(ay));
}
IC_DEV int select_mv_cand(int mx, int my)  // against L->pu.mv_cand
{
  const PuSearch &pu = L->pu;
  if (pu.mv_cand[0][0] == pu.mv_cand[1][0] && pu.mv_cand[0][1] == pu.mv_cand[1][1]) return 0;
  return mvd_coding_bits(mx - pu.mv_cand[1][0], my - pu.mv_cand[1][1]) < mvd_coding_bits(mx - pu.mv_cand[0][0], my - pu.mv_cand[0][1]) ? 1 : 0;
}
IC_DEV int mvd_bits(int x, int y)  // quarter samples
{
  const PuSearch &pu = L->pu;
  const int c1 = mvd_coding_bits(x - pu.mv_cand[0][0], y - pu.mv_cand[0][1]);
  const bool same = pu.mv_cand[0][0] == pu.mv_cand[1][0] && pu.mv_cand[0][1] == pu.mv_cand[1][1];
  const int c2 = same ? c1 : mvd_coding_bits(x - pu.mv_cand[1][0], y - pu.mv_cand[1][1]);
  return c1 < c2 ? c1 : c2;
}

// the SADs of probes k0 .. k0 + n - 1 (integer displacements L->px / L->py) against the PU's source block (the staged quadrant) into L->sad: edge-replicated reference (image.c:407)
// The probes of a round do not depend on each other: a lane takes its samples of ALL of them in one sweep (groups of four, a short group repeating its last probe),
// so the reference loads of a round are in flight together instead of one probe's after the other's sum.
template <int N> IC_DEV void probe_group(int k0, int n)
{
  IC_COUNT(20);
  const PuSearch &pu = L->pu;
  const gu8 *rp = refp(0);
  const int wh = pu.w * pu.w, l2 = ilog2i(pu.w), W = K->ref_w, H = K->ref_h;  // the reference FRAME: the picture (a tile) lies at (tile_x, tile_y) in it
  const PView o = orgv(0, pu.x - cx, pu.y - cy);
  int ox[N], oy[N];
  for (int k = 0; k < N; k++) { const int kk = k0 + (k < n ? k : n - 1); ox[k] = K->tile_x + pu.x + L->px[kk]; oy[k] = K->tile_y + pu.y + L->py[kk]; }
  u32 part[N];
  for (int k = 0; k < N; k++) part[k] = 0;
  bool inside = true;
  for (int k = 0; k < N; k++) inside = inside && ox[k] >= 0 && oy[k] >= 0 && ox[k] + pu.w <= W && oy[k] + pu.w <= H;
  if (inside) {  // every probe's block inside the reference frame: four samples per load (whatever the alignment) and per v_sad_u8
    int off[N];  // 32-bit offsets behind the one plane pointer (a frame is far below 2^31 samples): the load takes the pointer as its scalar base
    for (int k = 0; k < N; k++) off[k] = mul24v(oy[k], W) + ox[k];
    IC_FOR(tid) {
      for (int i = tid; i < (wh >> 2); i += KVZ_ICTU_THREADS) {
        const int yy = i >> (l2 - 2), x4 = (i & ((pu.w >> 2) - 1)) << 2;
        const u32 cur = lds_read32(o.p + yy * o.s + x4);
        const int row = mul24(yy, W) + x4;
        u32 r[N];
        for (int k = 0; k < N; k++) r[k] = glb_read32u(rp + (row + off[k]));
        for (int k = 0; k < N; k++) part[k] = sad4(cur, r[k], part[k]);
      }
    }
  } else
  IC_FOR(tid) {
    for (int i = tid; i < wh; i += KVZ_ICTU_THREADS) {
      const int yy = i >> l2, xx = i & (pu.w - 1), cur = (int)o.p[yy * o.s + xx];
      int r[N];
      for (int k = 0; k < N; k++) r[k] = rp[mul24(iclip(0, H - 1, oy[k] + yy), W) + iclip(0, W - 1, ox[k] + xx)];
      for (int k = 0; k < N; k++) part[k] += (u32)iabs(cur - r[k]);
    }
  }
  for (int k = 0; k < N; k++) { const u32 s = lanes_sum(part[k]); if (k < n) L->sad[k0 + k] = s; }
}
// ... and what check_mv_cost (search_inter.c:180-232) needs of a probe besides its SAD -- is the vector allowed, the MVD bits against the cheaper predictor -- by lane k for
// probe k, in the same phase: L->pbits[k] (-1: not allowed)
IC_FN void probe(int n)
{
#ifdef KVZ_ICTU_PROFILE_ME  /* developer build: the two halves of a probe round on the stage clock's spare slots (context copies = the bits, zero-coeff = loads + SADs) */
  auto bits_half = [&]() { IC_FOR(tid) { if (tid < n) { const int x = L->px[tid] * 4; const int y = L->py[tid] * 4; L->pbits[tid] = mv_allowed(x, y) ? mvd_bits(x, y) : -1; } } IC_SYNC(); };
  auto sad_half = [&]() { if (n > 4 && L->pu.w <= 16) probe_group<8>(0, n); else for (int k0 = 0; k0 < n; k0 += 4) probe_group<4>(k0, n - k0 < 4 ? n - k0 : 4); IC_SYNC(); };
  IC_PROF(IP_CTX, bits_half());
  IC_PROF(IP_ZERO_COEFF, sad_half());
  return;
#endif
  IC_FOR(tid) { if (tid < n) { const int x = L->px[tid] * 4, y = L->py[tid] * 4; L->pbits[tid] = mv_allowed(x, y) ? mvd_bits(x, y) : -1; } }
  if (n > 4 && L->pu.w <= 16) probe_group<8>(0, n);  // n <= 8; a 32x32 PU has sixteen samples per lane and probe: groups of four keep the sweep in registers
  else for (int k0 = 0; k0 < n; k0 += 4) probe_group<4>(k0, n - k0 < 4 ? n - k0 : 4);
  IC_SYNC();
}
struct MeBest { int mvx, mvy; double cost, bits; };
IC_DEV bool consider(MeBest &best, double lambda_sqrt, int k)  // check_mv_cost on probe k
{
  const int b = L->pbits[k];
  if (b < 0) return false;
  double cost = (double)L->sad[k];
  if (cost + 0.001 >= best.cost) return false;
  const double bits = (double)b;
  cost += bits * lambda_sqrt;
  if (cost + 0.001 >= best.cost) return false;
  best.mvx = L->px[k] * 4; best.mvy = L->py[k] * 4; best.cost = cost; best.bits = bits;
  return true;
}

// rows x cols samples of plane c of the reference picture from (X0, Y0) on into L->win, edge-replicated (kvz_get_extended_block, ipol-generic.c:761-814): whole
// dwords from the dword-aligned column at or before X0 while the window lies inside the picture, byte by byte with clamped addresses where it does not.
// Sample (r, cc) is win[r * IC_WS + L->win_xo + cc].
// (X0, Y0): position in the PICTURE; the window is read from the reference frame at the picture's offset in it and replicated at the frame's edges
IC_FN void stage_window(int c, int X0, int Y0, int rows, int cols)
{
  IC_COUNT(21);
  const int sh = c ? 1 : 0, fw = K->ref_w >> sh, fh = K->ref_h >> sh;
  X0 += K->tile_x >> sh; Y0 += K->tile_y >> sh;
  const gu8 *rp = refp(c);
  const int X0a = X0 & ~3, xo = X0 - X0a, ndw = (xo + cols + 3) >> 2;
  if (X0a >= 0 && X0a + 4 * ndw <= fw && Y0 >= 0 && Y0 + rows <= fh && (fw & 3) == 0 && ((size_t)rp & 3) == 0) {
    const unsigned md = div_magic(ndw);
    IC_FOR(tid) {
      for (int i = tid; i < rows * ndw; i += KVZ_ICTU_THREADS) {
        const int r = div_by(i, md), d = i - mul24(r, ndw);
        *(KVZ_LDS u32 *)(L->win + r * IC_WS + 4 * d) = *(const KVZ_GLB u32 *)(rp + (mul24(Y0 + r, fw) + X0a + 4 * d));
      }
    }
  } else {
    const unsigned mc = div_magic(cols);
    IC_FOR(tid) {
      for (int i = tid; i < rows * cols; i += KVZ_ICTU_THREADS) {
        const int r = div_by(i, mc), cc = i - mul24(r, cols);
        L->win[r * IC_WS + xo + cc] = rp[mul24(iclip(0, fh - 1, Y0 + r), fw) + iclip(0, fw - 1, X0 + cc)];
      }
    }
  }
  IC_FOR(tid) { if (tid == 0) L->win_xo = xo; }
  IC_SYNC();
}
// The horizontal pass of an interpolation (8 luma / 4 chroma taps, filter `fi` of K->luma_filter / K->chroma_filter) over the staged window: outputs (r, c), r < rows,
// c < cols, = sum_k f[k] * sample(r, c + k) into L->g[r * IC_GS + c].  A lane takes runs of four adjacent outputs: the run's bytes from whole dwords, shifted once to the
// run's first byte, the taps as two (one) v_dot4_i32_i8 on samples biased by -128 -- every filter sums to 64, so 128 * 64 goes back in.  The same integers as the plain sum.
IC_FN void hor_pass(int fi, int taps, int rows, int cols)
{
  const u32 f0 = taps == 8 ? *(const KVZ_LDS u32 *)&K->luma_filter[fi][0] : *(const KVZ_LDS u32 *)&K->chroma_filter[fi][0];
  const u32 f1 = taps == 8 ? *(const KVZ_LDS u32 *)&K->luma_filter[fi][4] : 0u;
  const int runs = (cols + 3) >> 2, xo = L->win_xo;
  const unsigned mr = div_magic(runs);
  IC_FOR(tid) {
    for (int t = tid; t < rows * runs; t += KVZ_ICTU_THREADS) {
      const int r = div_by(t, mr), c0 = (t - mul24(r, runs)) * 4, o = xo + c0, sh0 = o & 3;
      const KVZ_LDS u32 *p = (const KVZ_LDS u32 *)(L->win + r * IC_WS + (o & ~3));
      const u32 d0 = p[0] ^ 0x80808080u, d1 = p[1] ^ 0x80808080u, d2 = p[2] ^ 0x80808080u, d3 = taps == 8 ? p[3] ^ 0x80808080u : 0u;
      const u32 e0 = alignbyte(d1, d0, (u32)sh0), e1 = alignbyte(d2, d1, (u32)sh0), e2 = alignbyte(d3, d2, (u32)sh0);
      for (int j = 0; j < 4; j++) {
        int g = dot4(alignbyte(e1, e0, (u32)j), f0, 128 * 64);
        if (taps == 8) g = dot4(alignbyte(e2, e1, (u32)j), f1, g);
        if (c0 + j < cols) L->g[r * IC_GS + c0 + j] = (i16)g;
      }
    }
  }
  IC_SYNC();
}

// The vertical pass over L->g: out(y, x, v) for the w x w outputs v = (sum_j vf[j] * g[(y + ro + j) * IC_GS + x + co]) >> 6, vf = filter `fi`.  A lane takes four outputs of
// a column: TAPS + 3 intermediates read once instead of 4 x TAPS, the taps in registers.
template <int TAPS, class Out> IC_DEV void ver_pass(int fi, int ro, int co, int w, Out out)
{
  int vf[TAPS];
  for (int k = 0; k < TAPS; k++) vf[k] = TAPS == 8 ? K->luma_filter[fi][k] : K->chroma_filter[fi][k];
  const int l2 = ilog2i(w);
  IC_FOR(tid) {
    for (int t = tid; t < (w * w) >> 2; t += KVZ_ICTU_THREADS) {
      const int x = t & (w - 1), y0 = (t >> l2) << 2;
      int s[TAPS + 3];
      for (int k = 0; k < TAPS + 3; k++) s[k] = (int)L->g[(y0 + ro + k) * IC_GS + x + co];
      for (int j = 0; j < 4; j++) {
        int a = 0;
        for (int i = 0; i < TAPS; i++) a += vf[i] * s[j + i];
        out(y0 + j, x, a >> 6);
      }
    }
  }
}

// Tiles of L->pu: one of w x w, or the four 16x16 quadrants of a 32x32 PU
IC_DEV int tile_width(int w) { return w > 16 ? 16 : w; }
// the (tw + 8)^2 window of tile (tx, ty) around integer displacement (mx, my) of L->pu into L->win
IC_FN void load_frac_window(int mx, int my, int tx, int ty)
{
  const int tw = tile_width(L->pu.w);
  stage_window(0, L->pu.x + mx - 4 + tx * tw, L->pu.y + my - 4 + ty * tw, tw + 8, tw + 8);
}
// the SATD of L->pu at integer displacement (mx, my) against its source block, tile by tile (the last tile's window stays staged: a PU of one tile goes on from it)
IC_FN u32 satd_integer(int mx, int my)
{
  const int w = L->pu.w, tw = tile_width(w), nt = w > 16 ? w >> 4 : 1, l2 = ilog2i(tw);
  u32 total = 0;
  for (int ty = 0; ty < nt; ty++)
    for (int tx = 0; tx < nt; tx++) {
      load_frac_window(mx, my, tx, ty);
      const int xo = L->win_xo;
      IC_FOR(tid) { for (int i = tid; i < tw * tw; i += KVZ_ICTU_THREADS) { const int y = i >> l2, x = i & (tw - 1); L->pred[0][i] = L->win[(y + 4) * IC_WS + xo + x + 4]; } }
      IC_SYNC();
      const PView o = orgv(0, L->pu.x - cx + tx * tw, L->pu.y - cy + ty * tw);
      total += satd_block((const lu8 *)L->pred[0], tw, o.p, o.s, tw);
    }
  return total;
}

// the search patterns as packed constants, three bits per entry (value + 2): a local array indexed at run time would live in memory
IC_DEV int pat(unsigned long long packed, int i) { return (int)((packed >> (3 * i)) & 7ull) - 2; }
#define IC_PAT9(a, b, c, d, e, f, g, h, i) ((unsigned long long)((a) + 2) | (unsigned long long)((b) + 2) << 3 | (unsigned long long)((c) + 2) << 6 | (unsigned long long)((d) + 2) << 9 | \
                                            (unsigned long long)((e) + 2) << 12 | (unsigned long long)((f) + 2) << 15 | (unsigned long long)((g) + 2) << 18 | (unsigned long long)((h) + 2) << 21 | (unsigned long long)((i) + 2) << 24)

#if KVZ_ICTU_ME_STATE
// ---- the launch's choice of integer search (the ME builds, kvz_inter_ctu.hpp KVZ_ICTU_ME): what search_inter.c:1341-1383 runs behind select_starting_point ----
#ifdef KVZ_HOSTSIM
// what the searches met, for the script that chooses the fixture's clips (tests/golden/make_inter_me_golden.py): 0 TZ's second step 2 from zero, 1 a star refinement of
// two or more rounds, 2 a TZ round at distance >= 16 that improved, 3 / 4 the full search's window around the best vector run / left out, 5 a merge-candidate window
// with points an earlier window covered, 6 probes mv_allowed refused, 7 .. 10 a window that leaves the frame at its left / right / top / bottom, 11 / 12 a step limit
// that ended a diamond / hexagon loop which would have gone on, 13 sweeps, 14 acceptances inside sweeps
#define IC_ME_EVENT(slot) (++g_me_events[slot])
#define IC_LANES(type, name) type name[KVZ_ICTU_THREADS]
#define IC_LANE(name) name[tid]
#else
#define IC_ME_EVENT(slot)
#define IC_LANES(type, name) type name
#define IC_LANE(name) name
#endif
#define IC_ME_LOOP_BOUND (1 << 28)  /* a vector has at most 2^14 integer positions per axis and no centre comes twice (every move lowered the cost): no loop below takes more rounds */
struct MeWin { int x0, y0, x1, y1; };  // a window of integer displacements, its corners included
IC_DEV MeWin me_window(int mx, int my, int range) { return MeWin{ mx - range, my - range, mx + range, my + range }; }
IC_DEV MeWin me_seen(int j) { const KVZ_LDS int *s = me_windows() + 4 * j; return MeWin{ s[0], s[1], s[2], s[3] }; }
IC_DEV void me_see(int j, const MeWin &w) { KVZ_LDS int *s = me_windows() + 4 * j; IC_FOR(tid) { if (tid == 0) { s[0] = w.x0; s[1] = w.y0; s[2] = w.x1; s[3] = w.y1; } } }
IC_DEV bool me_in_window(const MeWin &w, int x, int y) { return x >= w.x0 && x <= w.x1 && y >= w.y0 && y <= w.y1; }
// probe k of L->px / L->py through check_mv_cost, counting refusals
IC_DEV bool me_consider(MeBest &best, double lambda_sqrt, int k)
{
  if (L->pbits[k] < 0) IC_ME_EVENT(6);
  return consider(best, lambda_sqrt, k);
}
// The full search's window `win` of integer displacements through check_mv_cost in raster order, A DISPLACEMENT PER LANE: the window's points are numbered row by
// row, sixty-four consecutive ones go to the sixty-four lanes, and a lane sums its whole block -- the source row is one LDS address for all lanes, the reference is
// read as unaligned dwords straight from the picture (v_sad_u8), byte by byte with clamped addresses where the lane's block leaves the reference frame; nothing is
// reduced across lanes.  Points inside one of the first n_skip windows of me_windows() were probed before and are left out (search_inter.c:941-959; probing them again could not
// be accepted).  The decision is check_mv_cost's, one probe after the other: a probe is accepted when its cost + 0.001 lies below the best so far, so the first lane
// that qualifies is taken, the best moves there, and the lanes are asked again until none qualifies -- the raster-order result in as many steps as there were
// improvements (the SAD-only test of check_mv_cost is implied: the bits only add to the cost).
IC_DEV KVZ_LDS int *me_windows() { return (KVZ_LDS int *)L->g; }  // the windows probed so far, [6] x {x0, y0, x1, y1}: L->g is dead while the integer search runs (the SATD and the interpolation come after it)
IC_FN void sweep_window(MeBest &best, double lambda_sqrt, const MeWin win, int n_skip)
{
  const PuSearch &pu = L->pu;
  const gu8 *rp = refp(0);
  const int w = pu.w, W = K->ref_w, H = K->ref_h, width = win.x1 - win.x0 + 1, points = width * (win.y1 - win.y0 + 1);
  const int bx = K->tile_x + pu.x, by = K->tile_y + pu.y;
  const PView o = orgv(0, pu.x - cx, pu.y - cy);
  IC_ME_EVENT(13);
  if (bx + win.x0 < 0) IC_ME_EVENT(7);
  if (bx + win.x1 + w > W) IC_ME_EVENT(8);
  if (by + win.y0 < 0) IC_ME_EVENT(9);
  if (by + win.y1 + w > H) IC_ME_EVENT(10);
  IC_LANES(int, lx); IC_LANES(int, ly);  // the lane's displacement: point chunk * 64 + lane of the window
  IC_FOR(tid) {
    int x = win.x0 + tid, y = win.y0;
    for (int k = 0; k < 4; k++) if (x > win.x1) { x -= width; y++; }  // (a window is at least 17 wide: 63 is fewer than four rows)
    IC_LANE(lx) = x; IC_LANE(ly) = y;
  }
  for (int p0 = 0; p0 < points; p0 += KVZ_ICTU_THREADS) {
    IC_LANES(u32, lsad); IC_LANES(int, lbits);
    IC_FOR(tid) {
      const int x = IC_LANE(lx), y = IC_LANE(ly);
      bool live = p0 + tid < points;
      for (int j = 0; j < n_skip; j++) { const MeWin sw = me_seen(j); live = live && !me_in_window(sw, x, y); }
      int bits = -1;
      u32 sad = 0;
      if (live) {
        if (mv_allowed(x * 4, y * 4)) bits = mvd_bits(x * 4, y * 4); else IC_ME_EVENT(6);
      }
      if (bits >= 0) {
        const int ox = bx + x, oy = by + y;
        if (ox >= 0 && oy >= 0 && ox + w <= W && oy + w <= H) {  // the lane's block inside the reference frame
          const int off = mul24(oy, W) + ox;
          for (int yy = 0; yy < w; yy++) {
            const int row = mul24(yy, W) + off;
            for (int x4 = 0; x4 < w; x4 += 4) sad = sad4(lds_read32(o.p + yy * o.s + x4), glb_read32u(rp + (row + x4)), sad);
          }
        } else {
          for (int yy = 0; yy < w; yy++) {
            const int row = mul24(iclip(0, H - 1, oy + yy), W);
            for (int xx = 0; xx < w; xx++) sad += (u32)iabs((int)o.p[yy * o.s + xx] - (int)rp[row + iclip(0, W - 1, ox + xx)]);
          }
        }
      }
      IC_LANE(lsad) = sad; IC_LANE(lbits) = bits;
    }
    for (int taken = 0; taken <= KVZ_ICTU_THREADS; taken++) {  // (every acceptance takes a later lane or ends the loop: never more rounds than lanes)
      int first = -1;
#ifdef KVZ_HOSTSIM
      for (int l = KVZ_ICTU_THREADS - 1; l >= 0; l--) if (lbits[l] >= 0 && (double)lsad[l] + (double)lbits[l] * lambda_sqrt + 0.001 < best.cost) first = l;
#else
      const unsigned long long ask = __builtin_amdgcn_ballot_w64(lbits >= 0 && (double)lsad + (double)lbits * lambda_sqrt + 0.001 < best.cost);
      if (ask) first = (int)__builtin_ctzll(ask);
#endif
      if (first < 0) break;
      IC_ME_EVENT(14);
#ifdef KVZ_HOSTSIM
      const u32 s = lsad[first]; const int b = lbits[first], fx = lx[first], fy = ly[first];
#else
      const u32 s = (u32)__builtin_amdgcn_readlane((int)lsad, first); const int b = __builtin_amdgcn_readlane(lbits, first), fx = __builtin_amdgcn_readlane(lx, first), fy = __builtin_amdgcn_readlane(ly, first);
#endif
      best.mvx = fx * 4; best.mvy = fy * 4; best.bits = (double)b; best.cost = (double)s + (double)b * lambda_sqrt;
    }
    IC_FOR(tid) {  // on to the lane's point of the next chunk
      int x = IC_LANE(lx) + KVZ_ICTU_THREADS, y = IC_LANE(ly);
      for (int k = 0; k < 4; k++) if (x > win.x1) { x -= width; y++; }
      IC_LANE(lx) = x; IC_LANE(ly) = y;
    }
  }
}
// search_mv_full (search_inter.c:892-965) on L->best: the window around zero, the one around the vector the search is entered with unless that is a merge candidate's, and one
// around every merge candidate of a single list -- its vector cut with >> 2 here, not rounded as select_starting_point rounds it -- without the points of the zero
// window and of the earlier candidates' windows.  One call (the windows of a search share one copy of the sweep).
IC_FN_CALL void me_full(int range)
{
  const PuSearch &pu = L->pu;
  const double lambda_sqrt = M->lambda_sqrt;
  MeBest best{ L->best.mvx, L->best.mvy, L->best.cost, L->best.bits };
  int n_seen = 0;
  const int ex = best.mvx >> 2, ey = best.mvy >> 2;  // (extra_mv is the best vector the search was entered with)
  for (int k = 0; k < 2 + pu.num_merge; k++) {  // 0: zero; 1: the best vector on entry; 2 ..: merge candidate k - 2
    MeWin win = me_window(0, 0, range);
    int skip = 0;
    if (k == 1) {
      bool in_merge = false;
      for (int i = 0; i < pu.num_merge; i++) {
        const MCand c = pu.merge[i];
        const int cmx = c.dir == 1 ? c.mv[0][0] : c.mv[1][0], cmy = c.dir == 1 ? c.mv[0][1] : c.mv[1][1];
        if (c.dir != 3 && ((cmx + 2) >> 2) == ex && ((cmy + 2) >> 2) == ey) in_merge = true;
      }
      if (in_merge) { IC_ME_EVENT(4); continue; }
      IC_ME_EVENT(3);
      win = me_window(ex, ey, range);
    } else if (k >= 2) {
      const MCand c = pu.merge[k - 2];
      if (c.dir == 3) continue;
      const int mx = (c.dir == 1 ? c.mv[0][0] : c.mv[1][0]) >> 2, my = (c.dir == 1 ? c.mv[0][1] : c.mv[1][1]) >> 2;
      win = me_window(mx, my, range);
      skip = n_seen;
      me_see(n_seen, win);  // (its own window is not among the `skip` ones it is swept without)
      n_seen++;
      if (mx == 0 && my == 0) continue;
#ifdef KVZ_HOSTSIM
      for (int j = 0; j < skip; j++) { const MeWin sj = me_seen(j); if (win.x0 <= sj.x1 && win.x1 >= sj.x0 && win.y0 <= sj.y1 && win.y1 >= sj.y0) { IC_ME_EVENT(5); break; } }
#endif
    } else {
      me_see(0, win);
      n_seen = 1;
    }
    IC_SYNC();
    sweep_window(best, lambda_sqrt, win, skip);
  }
  IC_FOR(tid) { if (tid == 0) { L->best.mvx = best.mvx; L->best.mvy = best.mvy; L->best.cost = best.cost; L->best.bits = best.bits; } }
  IC_SYNC();
}
// one round of kvz_tz_pattern_search with the diamond pattern (search_inter.c:487-604, type 0) at distance d around (mx, my): true when a point was accepted
IC_FN bool me_tz_round(MeBest &best, double lambda_sqrt, int mx, int my, int d)
{
  const int h = d >> 1, n = d == 1 ? 4 : 8;
  i16 *px = L->px, *py = L->py;
  px[0] = mx; py[0] = my + d; px[1] = mx + d; py[1] = my; px[2] = mx; py[2] = my - d; px[3] = mx - d; py[3] = my;
  px[4] = mx + h; py[4] = my + h; px[5] = mx + h; py[5] = my - h; px[6] = mx - h; py[6] = my - h; px[7] = mx - h; py[7] = my + h;
  probe(n);
  bool any = false;
  for (int j = 0; j < n; j++) if (me_consider(best, lambda_sqrt, j)) any = true;
  if (any && d >= 16) IC_ME_EVENT(2);
  return any;
}
// tz_search (search_inter.c:625-693) as the reference's compile-time switches leave it: step 2 from the best vector, step 2 from zero up to half the range when the
// start was not zero, the star refinement; best_dist travels through all three
IC_FN void me_tz(MeBest &best, double lambda_sqrt)
{
  const int range = 96;
  int best_dist = 0;
  const int sx0 = best.mvx >> 2, sy0 = best.mvy >> 2;
  for (int part = 0; part < 2; part++) {
    if (part == 1) { if (sx0 == 0 && sy0 == 0) break; IC_ME_EVENT(0); }
    int idle = 0;
    for (int d = 1; d <= (part ? range / 2 : range); d *= 2) {
      if (me_tz_round(best, lambda_sqrt, part ? 0 : sx0, part ? 0 : sy0, d)) best_dist = d;
      if (best_dist != d) idle++;
      if (idle >= 3) break;
    }
  }
  int rounds = 0;
  while (best_dist > 0) {
    if (++rounds > IC_ME_LOOP_BOUND) { g_ic.me_overrun = 1; break; }
    if (rounds == 2) IC_ME_EVENT(1);
    best_dist = 0;
    const int mx = best.mvx >> 2, my = best.mvy >> 2;
    for (int d = 1; d <= range; d *= 2) if (me_tz_round(best, lambda_sqrt, mx, my, d)) best_dist = d;
  }
}
// diamond_search (search_inter.c:810-889): five points, the centre among them; then three per round, without the one at index best_index ^ 3 of the last move
IC_FN void me_diamond(MeBest &best, double lambda_sqrt, int max_steps)
{
  const unsigned long long dx = IC_PAT9(0, 1, 0, -1, 0, 0, 0, 0, 0), dy = IC_PAT9(-1, 0, 1, 0, 0, 0, 0, 0, 0);
  i16 *px = L->px, *py = L->py;
  int mx = best.mvx >> 2, my = best.mvy >> 2, best_index = 4;
  for (int j = 0; j < 5; j++) { px[j] = mx + pat(dx, j); py[j] = my + pat(dy, j); }
  probe(5);
  for (int j = 0; j < 5; j++) if (me_consider(best, lambda_sqrt, j)) best_index = j;
  if (best_index == 4) return;
  mx += pat(dx, best_index); my += pat(dy, best_index);
  int from_dir = 4, steps = max_steps;
  for (int rounds = 0;; rounds++) {
    if (rounds >= IC_ME_LOOP_BOUND) { g_ic.me_overrun = 1; break; }
    bool better = false;
    if (steps > 0) steps--;
    int n = 0, idx[4];
    for (int i = 0; i < 4; i++) if (i != from_dir) { px[n] = mx + pat(dx, i); py[n] = my + pat(dy, i); idx[n] = i; n++; }
    probe(n);
    for (int j = 0; j < n; j++) if (me_consider(best, lambda_sqrt, j)) { best_index = idx[j]; better = true; }
    if (better) { mx += pat(dx, best_index); my += pat(dy, best_index); from_dir = best_index ^ 3; }
    if (!better) break;
    if (max_steps > 0 && steps == 0) { IC_ME_EVENT(11); break; }
  }
}
#endif

// search_pu_inter_ref's search (oracle me_integer) for L->pu into L->best; (sx, sy): the co-located motion, if has_start
IC_FN void me_integer(bool has_start, int sx, int sy)
{
  const PuSearch &pu = L->pu;
  i16 *px = L->px, *py = L->py;
  MeBest best{ 0, 0, IC_MAX_COST, IC_MAX_INT };  // check_mv_cost's best so far, in registers
  const double lambda_sqrt = M->lambda_sqrt;
  int ex = 0, ey = 0;
  if (has_start && mv_allowed(sx, sy)) { ex = sx; ey = sy; }
  best.mvx = ex; best.mvy = ey;
  ex >>= 2; ey >>= 2;
  {  // select_starting_point
    int n = 0;
    px[n] = 0; py[n] = 0; n++;
    bool extra = ex != 0 || ey != 0;
    if (extra)
      for (int i = 0; i < pu.num_merge; i++) {
        const MCand c = pu.merge[i];
        const int cmx = c.dir == 1 ? c.mv[0][0] : c.mv[1][0], cmy = c.dir == 1 ? c.mv[0][1] : c.mv[1][1];  // (a select: an index computed at run time puts the record on the stack)
        if (c.dir != 3 && ((cmx + 2) >> 2) == ex && ((cmy + 2) >> 2) == ey) { extra = false; break; }
      }
    if (extra) { px[n] = ex; py[n] = ey; n++; }
    for (int i = 0; i < pu.num_merge; i++) {
      const MCand c = pu.merge[i];
      if (c.dir == 3) continue;
      const int x = ((c.dir == 1 ? c.mv[0][0] : c.mv[1][0]) + 2) >> 2, y = ((c.dir == 1 ? c.mv[0][1] : c.mv[1][1]) + 2) >> 2;
      if (x == 0 && y == 0) continue;
      px[n] = x; py[n] = y; n++;
    }
    probe(n);
    for (int k = 0; k < n; k++) consider(best, lambda_sqrt, k);
  }
  bool skip_me = false;
#if KVZ_ICTU_ME_STATE
  if (KVZ_ICTU_ME) {  // the launch's own choice (search_inter.c:1341-1383)
    const int algo = M->me_algorithm, term = M->me_early_termination, max_steps = M->me_max_steps;
    {  // early_terminate (search_inter.c:436-484) runs whatever the setting -- it moves the best vector --, `off` (2) only ignores its verdict; `on` (1): the best cost itself is the threshold
      const unsigned long long hx = IC_PAT9(0, -1, 0, 1, 0, -1, 0, 0, 0), hy = IC_PAT9(-1, 0, 1, 0, -1, 0, 0, 0, 0);
      int mx = best.mvx >> 2, my = best.mvy >> 2, first = 0, last = 3;
      for (int k = 0; k < 2; k++) {
        const double threshold = term == 0 ? best.cost * 0.95 : best.cost;
        int best_index = 6;
        const int n = last - first + 1;
        for (int j = 0; j < n; j++) { px[j] = mx + pat(hx, first + j); py[j] = my + pat(hy, first + j); }
        probe(n);
        for (int j = 0; j < n; j++) if (me_consider(best, lambda_sqrt, j)) best_index = first + j;
        mx += pat(hx, best_index); my += pat(hy, best_index);
        if (best.cost >= threshold) { skip_me = true; break; }
        first = (best_index + 3) % 4;
        last = first + 2;
      }
    }
    if (term == 2) skip_me = false;
    if (skip_me) {
    } else if (algo == 1) me_tz(best, lambda_sqrt);
    else if (algo >= 2 && algo <= 6) {
      IC_FOR(tid) { if (tid == 0) { L->best.mvx = best.mvx; L->best.mvy = best.mvy; L->best.cost = best.cost; L->best.bits = best.bits; } }
      IC_SYNC();
      me_full(algo == 3 ? 8 : (algo == 4 ? 16 : (algo == 6 ? 64 : 32)));
      best.mvx = L->best.mvx; best.mvy = L->best.mvy; best.cost = L->best.cost; best.bits = L->best.bits;
    } else if (algo == 7) me_diamond(best, lambda_sqrt, max_steps);
    else {  // hexagon_search with --me-steps (search_inter.c:712-792): the limit counts the moves of the large hexagon, the small one always runs
      const unsigned long long lx = IC_PAT9(0, 1, 2, 1, -1, -2, -1, 1, 2), ly = IC_PAT9(0, -2, 0, 2, 2, 0, -2, -2, 0);
      const unsigned long long sx9 = IC_PAT9(0, 0, -1, 1, 0, -1, 1, -1, 1), sy9 = IC_PAT9(0, -1, 0, 0, 1, -1, -1, 1, 1);
      int mx = best.mvx >> 2, my = best.mvy >> 2, best_index = 0, steps = max_steps, rounds = 0;
      for (int j = 0; j < 6; j++) { px[j] = mx + pat(lx, j + 1); py[j] = my + pat(ly, j + 1); }
      probe(6);
      for (int j = 0; j < 6; j++) if (me_consider(best, lambda_sqrt, j)) best_index = j + 1;
      while (best_index != 0) {
        if (max_steps > 0 && steps == 0) { IC_ME_EVENT(12); break; }
        if (++rounds > IC_ME_LOOP_BOUND) { g_ic.me_overrun = 1; break; }
        if (steps > 0) steps--;
        const int start_i = best_index == 1 ? 6 : (best_index == 8 ? 1 : best_index - 1);
        mx += pat(lx, best_index); my += pat(ly, best_index);
        best_index = 0;
        for (int j = 0; j < 3; j++) { px[j] = mx + pat(lx, start_i + j); py[j] = my + pat(ly, start_i + j); }
        probe(3);
        for (int j = 0; j < 3; j++) if (me_consider(best, lambda_sqrt, j)) best_index = start_i + j;
      }
      for (int j = 0; j < 8; j++) { px[j] = mx + pat(sx9, j + 1); py[j] = my + pat(sy9, j + 1); }
      probe(8);
      for (int j = 0; j < 8; j++) me_consider(best, lambda_sqrt, j);
    }
    skip_me = true;  // (nothing of the default search below)
  } else
#endif
  {  // early_terminate, sensitive (search_inter.c:425-486): the small cross, entries first .. last
    const unsigned long long hx = IC_PAT9(0, -1, 0, 1, 0, -1, 0, 0, 0), hy = IC_PAT9(-1, 0, 1, 0, -1, 0, 0, 0, 0);
    int mx = best.mvx >> 2, my = best.mvy >> 2, first = 0, last = 3;
    for (int k = 0; k < 2; k++) {
      const double threshold = best.cost * 0.95;
      int best_index = 6;
      const int n = last - first + 1;
      for (int j = 0; j < n; j++) { px[j] = mx + pat(hx, first + j); py[j] = my + pat(hy, first + j); }
      probe(n);
      for (int j = 0; j < n; j++) if (consider(best, lambda_sqrt, j)) best_index = first + j;
      mx += pat(hx, best_index); my += pat(hy, best_index);
      if (best.cost >= threshold) { skip_me = true; break; }
      first = (best_index + 3) % 4;
      last = first + 2;
    }
  }
  if (!skip_me) {  // hexagon_search (search_inter.c:712-800)
    const unsigned long long lx = IC_PAT9(0, 1, 2, 1, -1, -2, -1, 1, 2), ly = IC_PAT9(0, -2, 0, 2, 2, 0, -2, -2, 0);
    const unsigned long long sx9 = IC_PAT9(0, 0, -1, 1, 0, -1, 1, -1, 1), sy9 = IC_PAT9(0, -1, 0, 0, 1, -1, -1, 1, 1);
    int mx = best.mvx >> 2, my = best.mvy >> 2, best_index = 0;
    for (int j = 0; j < 6; j++) { px[j] = mx + pat(lx, j + 1); py[j] = my + pat(ly, j + 1); }
    probe(6);
    for (int j = 0; j < 6; j++) if (consider(best, lambda_sqrt, j)) best_index = j + 1;
    while (best_index != 0) {
      const int start_i = best_index == 1 ? 6 : (best_index == 8 ? 1 : best_index - 1);
      mx += pat(lx, best_index); my += pat(ly, best_index);
      best_index = 0;
      for (int j = 0; j < 3; j++) { px[j] = mx + pat(lx, start_i + j); py[j] = my + pat(ly, start_i + j); }
      probe(3);
      for (int j = 0; j < 3; j++) if (consider(best, lambda_sqrt, j)) best_index = start_i + j;
    }
    for (int j = 0; j < 8; j++) { px[j] = mx + pat(sx9, j + 1); py[j] = my + pat(sy9, j + 1); }
    probe(8);
    for (int j = 0; j < 8; j++) consider(best, lambda_sqrt, j);
  }
  if (M->fme_level == 0 && best.cost < IC_MAX_COST) {  // SATD at the integer position
    best.cost = (double)satd_integer(best.mvx >> 2, best.mvy >> 2);
    best.cost += best.bits * lambda_sqrt;
  }
  L->best.mvx = best.mvx; L->best.mvy = best.mvy; L->best.cost = best.cost; L->best.bits = best.bits;
}


// search_frac (oracle search_frac / me_fractional) of L->pu from the integer vector L->frac.mv: the two half-sample steps (fme_level 2) and the two quarter-sample steps
// around the best half-sample position (fme_level 4) into L->frac; returns false when no quarter-sample step is possible
IC_FN bool me_fractional()
{
  L->frac.cost = IC_MAX_COST; L->frac.bits = IC_MAX_INT;
  const int fmx = L->frac.mv[0], fmy = L->frac.mv[1];
  if (!mv_allowed(fmx + 3, fmy + 3) && !mv_allowed(fmx - 3, fmy - 3)) return false;
  const unsigned long long sqx = IC_PAT9(0, -1, 1, 0, 0, -1, 1, -1, 1), sqy = IC_PAT9(0, 0, 0, -1, 1, -1, -1, 1, 1);
  const int w = L->pu.w, tw = tile_width(w), nt = w > 16 ? w >> 4 : 1, l2t = ilog2i(tw);
  int mx = fmx >> 2, my = fmy >> 2;
  const int imx = mx, imy = my;
  double bitcost = (double)mvd_bits(mx * 4, my * 4);
  const u32 c0 = (u32)((double)satd_integer(mx, my) + bitcost * M->lambda_sqrt);
  double cost = (double)c0;
  mx *= 2; my *= 2;
  int best_index = 0, i0 = 1, off_x = 0, off_y = 0;
  const int steps = M->fme_level;
  for (int step = 0; step < steps; step++) {
    const int unit = step < 2 ? 2 : 1;  // quarter samples per step of this precision (mv_shift of search_inter.c:1090)
    FmePlane pl[4];
    fme_planes(step, off_x, off_y, pl);
    u32 sc[4] = { 0, 0, 0, 0 };
    for (int ty = 0; ty < nt; ty++)
      for (int tx = 0; tx < nt; tx++) {
        if (nt > 1) load_frac_window(imx, imy, tx, ty);  // (one tile: satd_integer left its window staged, and nothing has written L->win since)
        int done = 0;
        for (int first = 0; first < 4; first++) {
          if (done & (1 << first)) continue;
          const int hf = pl[first].hf;
          hor_pass(hf, 8, tw + 8, tw + 1);
          for (int p = first; p < 4; p++) {
            if (pl[p].hf != hf) continue;
            done |= 1 << p;
            lu8 *plane = (lu8 *)L->pred[p];
            ver_pass<8>(pl[p].vf, pl[p].roff, pl[p].coff, tw, [=](int y, int x, int v) { plane[(y << l2t) + x] = fin14(v); });
          }
          IC_SYNC();
        }
        {  // the four planes' SATDs: one item per (plane, 8x8 block of the tile)
          const PView org0 = orgv(0, L->pu.x - cx + tx * tw, L->pu.y - cy + ty * tw);
          const int bw = tw >> 3, blocks = bw * bw, l2b = ilog2i(bw);
          u32 part[4] = { 0, 0, 0, 0 };
          satd_tiles(4 * blocks, tw, org0.s,
                     [=](int it, const lu8 *&pa, const lu8 *&pb) {
                       const int p = it >> (2 * l2b), t = it & (blocks - 1), by = t >> l2b, bx = t & (bw - 1);
                       pa = (const lu8 *)L->pred[0] + p * 256 + by * 8 * tw + bx * 8; pb = org0.p + by * 8 * org0.s + bx * 8;
                     },
                     [&](int it, u32 v) { const int p = it >> (2 * l2b); part[0] += p == 0 ? v : 0; part[1] += p == 1 ? v : 0; part[2] += p == 2 ? v : 0; part[3] += p == 3 ? v : 0; });
          for (int p = 0; p < 4; p++) sc[p] += lanes_sum(part[p]);
        }
      }
    for (int j = 0; j < 4; j++) {
      const int cx_ = mx + pat(sqx, i0 + j), cy_ = my + pat(sqy, i0 + j);
      if (!mv_allowed(cx_ * unit, cy_ * unit)) continue;
      const double b = (double)mvd_bits(cx_ * unit, cy_ * unit);
      const u32 cj = (u32)((double)sc[j] + b * M->lambda_sqrt);
      if ((double)cj < cost) { cost = (double)cj; bitcost = b; best_index = i0 + j; }
    }
    i0 += 4;
    if (step == 1 || step == steps - 1) {  // search_inter.c:1146-1162: move to the best position of this precision, then on to quarter samples
      mx += pat(sqx, best_index); my += pat(sqy, best_index);
      if (step == (steps - 1 < 1 ? steps - 1 : 1)) { mx *= 2; my *= 2; off_x = pat(sqx, best_index); off_y = pat(sqy, best_index); best_index = 0; i0 = 1; }
    }
  }
  L->frac.mv[0] = mx; L->frac.mv[1] = my;
  L->frac.cost = cost; L->frac.bits = bitcost;
  return true;
}

// ---- motion-compensated prediction (oracle predict_list / inter_predict): the 2Nx2N PU of the w x w CU at (x, y), a tile at a time ----
// The horizontal pass of hor_pass STRAIGHT FROM THE REFERENCE PICTURE (no staging phase): rows x cols outputs, output (r, c) = sum_k f[k] * ref(Y0 + r, X0 + c + k).  Only
// where the window and the whole dwords a run reads (up to 12 bytes past its last tap) lie inside the plane's rows -- the caller checks with window_inside.
IC_DEV bool window_inside(int c, int X0, int Y0, int rows, int cols_taps)
{
  const int sh = c ? 1 : 0, fw = K->ref_w >> sh, fh = K->ref_h >> sh;
  X0 += K->tile_x >> sh; Y0 += K->tile_y >> sh;
  return X0 >= 0 && Y0 >= 0 && Y0 + rows <= fh && (X0 & ~3) + ((cols_taps + 6) & ~3) + 12 <= fw && (fw & 3) == 0 && ((size_t)refp(c) & 3) == 0;
}
IC_FN void hor_pass_ref(int c, int X0, int Y0, int fi, int taps, int rows, int cols)
{
  IC_COUNT(22);
  const int fw = K->ref_w >> (c ? 1 : 0);
  X0 += K->tile_x >> (c ? 1 : 0); Y0 += K->tile_y >> (c ? 1 : 0);
  const gu8 *rp = refp(c);
  const u32 f0 = taps == 8 ? *(const KVZ_LDS u32 *)&K->luma_filter[fi][0] : *(const KVZ_LDS u32 *)&K->chroma_filter[fi][0];
  const u32 f1 = taps == 8 ? *(const KVZ_LDS u32 *)&K->luma_filter[fi][4] : 0u;
  const int runs = (cols + 3) >> 2;
  const unsigned mr = div_magic(runs);
  IC_FOR(tid) {
    for (int t = tid; t < rows * runs; t += KVZ_ICTU_THREADS) {
      const int r = div_by(t, mr), c0 = (t - mul24(r, runs)) * 4, o = X0 + c0, sh0 = o & 3;
      const KVZ_GLB u32 *p = (const KVZ_GLB u32 *)(rp + (mul24(Y0 + r, fw) + (o & ~3)));
      const u32 d0 = p[0] ^ 0x80808080u, d1 = p[1] ^ 0x80808080u, d2 = p[2] ^ 0x80808080u, d3 = taps == 8 ? p[3] ^ 0x80808080u : 0u;
      const u32 e0 = alignbyte(d1, d0, (u32)sh0), e1 = alignbyte(d2, d1, (u32)sh0), e2 = alignbyte(d3, d2, (u32)sh0);
      for (int j = 0; j < 4; j++) {
        int g = dot4(alignbyte(e1, e0, (u32)j), f0, 128 * 64);
        if (taps == 8) g = dot4(alignbyte(e2, e1, (u32)j), f1, g);
        if (c0 + j < cols) L->g[r * IC_GS + c0 + j] = (i16)g;
      }
    }
  }
  IC_SYNC();
}
// One list, one plane, one tile: the tw x tw block at reference position (X0, Y0) [the integer part of the motion applied], fractional filters (hf, vf) (identity taps
// make every branch of inter_recon_unipred the same expression, kvz_fme.hpp).  What happens to the 14-bit sample v of (y, x): mode 0 -- into L->im[0] as int16; mode 1 --
// the finished sample of a prediction from one list, clip((v + 32) >> 6), v whole (kvz_sample_quarterpel_luma clips the int32: the luma (2, 2) phase reaches 33150);
// mode 2 -- that of two lists, clip((L->im[0] + int16(v) + 64) >> 7) (inter.c:374-660); mode 3 -- two lists with one vector predicted as one: the operands are
// int16(v) as in mode 2, clip((2 int16(v) + 64) >> 7) = clip((int16(v) + 32) >> 6).
IC_FN void predict_tile(int c, int X0, int Y0, int tw, int hf, int vf, int mode, lu8 *dst, int ds)
{
  IC_COUNT(23);
  if (hf == 0 && vf == 0) IC_COUNT(24); else if (hf == 0 || vf == 0) IC_COUNT(25);
  if (mode == 0 || mode == 2) IC_COUNT(26);
  const int taps = c ? 4 : 8, before = c ? 1 : 3, wr = tw + taps - 1, l2 = ilog2i(tw);
  if (hf == 0 && vf == 0) {
    // a whole-sample vector: both passes with the identity taps come to sample << 6 -- the block itself is all the window there is to read
    stage_window(c, X0, Y0, tw, tw);
    li16 *im0 = (li16 *)L->im[0];
    const int xo = L->win_xo;
    IC_FOR(tid) {
      for (int i = tid; i < tw * tw; i += KVZ_ICTU_THREADS) {
        const int yy = i >> l2, xx = i & (tw - 1), px = (int)L->win[yy * IC_WS + xo + xx];
        if (mode == 0) im0[i] = (i16)(px << 6);
        else if (mode != 2) dst[yy * ds + xx] = (u8)px;
        else dst[yy * ds + xx] = clip_pixel(((int)im0[i] + (px << 6) + 64) >> 7);
      }
    }
    IC_SYNC();
    return;
  }
  if (window_inside(c, X0 - before, Y0 - before, wr, wr)) hor_pass_ref(c, X0 - before, Y0 - before, hf, taps, wr, tw);
  else { stage_window(c, X0 - before, Y0 - before, wr, wr); hor_pass(hf, taps, wr, tw); }
  li16 *im = (li16 *)L->im[0];
  if (mode == 0) {
    if (c) ver_pass<4>(vf, 0, 0, tw, [=](int yy, int xx, int v) { im[(yy << l2) + xx] = (i16)v; });
    else ver_pass<8>(vf, 0, 0, tw, [=](int yy, int xx, int v) { im[(yy << l2) + xx] = (i16)v; });
  } else if (mode != 2) {
    const bool wrap = mode == 3;
    if (c) ver_pass<4>(vf, 0, 0, tw, [=](int yy, int xx, int v) { dst[yy * ds + xx] = clip_pixel(((wrap ? (int)(i16)v : v) + 32) >> 6); });
    else ver_pass<8>(vf, 0, 0, tw, [=](int yy, int xx, int v) { dst[yy * ds + xx] = clip_pixel(((wrap ? (int)(i16)v : v) + 32) >> 6); });
  } else {
    if (c) ver_pass<4>(vf, 0, 0, tw, [=](int yy, int xx, int v) { dst[yy * ds + xx] = clip_pixel(((int)im[(yy << l2) + xx] + (int)(i16)v + 64) >> 7); });
    else ver_pass<8>(vf, 0, 0, tw, [=](int yy, int xx, int v) { dst[yy * ds + xx] = clip_pixel(((int)im[(yy << l2) + xx] + (int)(i16)v + 64) >> 7); });
  }
  IC_SYNC();
}
// plane c of the prediction `pu` describes into dst (stride ds)
IC_DEV void predict_into(int c, int x, int y, int w, const CuInfo &pu, lu8 *dst, int ds)
{
  const int sh = c ? 1 : 0, bw = w >> sh, tw = tile_width(bw), nt = bw > 16 ? bw >> 4 : 1;
  for (int ty = 0; ty < nt; ty++)
    for (int tx = 0; tx < nt; tx++) {
      lu8 *d = dst + ty * tw * ds + tx * tw;
      // (both lists hold the one reference picture: two lists with one vector average a block with itself -- (2 v + 64) >> 7 = (v + 32) >> 6 -- predicted as one list
      // whose 14-bit samples are still the wrapped int16 operands of two: mode 3)
      // (a P slice predicts from list 0 and nothing else: no second list, nothing to recognise)
      const bool twice = !KVZ_ICTU_P && pu.mv_dir == 3 && pu.mv[0][0] == pu.mv[1][0] && pu.mv[0][1] == pu.mv[1][1];
      const int first = !KVZ_ICTU_P && pu.mv_dir == 2 ? 1 : 0, lists = !KVZ_ICTU_P && pu.mv_dir == 3 && !twice ? 2 : 1;
      if (twice) IC_COUNT(27);
      for (int k = 0; k < lists; k++) {
        const bool second = first + k != 0;
        const int mvx = second ? pu.mv[1][0] : pu.mv[0][0], mvy = second ? pu.mv[1][1] : pu.mv[0][1];
        predict_tile(c, (x >> sh) + (mvx >> (2 + sh)) + tx * tw, (y >> sh) + (mvy >> (2 + sh)) + ty * tw, tw, c ? mvx & 7 : mvx & 3, c ? mvy & 7 : mvy & 3, twice ? 3 : (lists == 1 ? 1 : (k == 0 ? 0 : 2)), d, ds);
      }
    }
}
// the luma prediction alone into level lv's samples: what a merge candidate's SATD is taken on
IC_FN void inter_predict(int lv, int x, int y, int w, const CuInfo pu, bool luma, bool chroma)
{
  const int xl = x - cx, yl = y - cy;
#if KVZ_ICTU_REFS_STATE
  if (KVZ_ICTU_REFS) use_ref(pu.mv_ref[0]);  // the picture the reference index names (inter.c:574-586); a P record moves by list 0
#endif
  for (int c = 0; c < 3; c++) {
    if ((c == 0 && !luma) || (c > 0 && !chroma)) continue;
    const PView dv = lvl(lv, c, xl, yl);
    predict_into(c, x, y, w, pu, dv.p, dv.s);
  }
}

// ---- one transform unit: kvz_quantize_residual (quant-generic.c:198-292) of the w x w block of plane c at LCU position (xl, yl) [luma coordinates] in level lv:
// prediction in the level's samples -> reconstruction there, levels into the level's coefficient array.  Returns has_coeffs; L->ccost[c] = kvz_fast_coeff_cost of the levels.
// One pass of the separable transform (dct-generic.c:255-629 as exact integer matrix products) IN PLACE on the W x W block x: every pass reads rows and writes columns,
//   out[m * W + j] = f((sum_i A[m][i] * in[j * W + i] + add) >> shift)
// forward (f = wrap to 16 bits) with A = C, the W-point matrix out of K->dct32 (its rows 0, 32 / W, ..: `rs` apart; or the DST): dst[k * n + j] = sum_i C[k][i] * src[j * n + i] as the
// reference's partial butterflies; inverse (f = clip to 16 bits) with A = C transposed on TRANSPOSED storage: the reference's dst[j * n + i] = sum_k C[k][i] * src[k * n + j] reads
// column j of its input and writes row j, so with every buffer of the inverse path held transposed (the dequantisation writes that way, the reconstruction reads that way)
// it is the same kernel.  A lane holds row j of the input in registers and computes the W * W / 64 outputs m = q, q + 64 / W, .. of column j; all lanes read before any writes.
// (IC_KEEP: what a lane computes in one phase and stores in the next lives in its registers; the host simulation, whose "lanes" run one after the other, keeps it per item)
#ifdef KVZ_HOSTSIM
#define IC_KEEP_DECL(name, per_lane, items) static int name[items]
#define IC_KEEP(name, t, item) name[item]
#else
#define IC_KEEP_DECL(name, per_lane, items) int name[per_lane]
#define IC_KEEP(name, t, item) name[t]
#endif
template <int W> IC_DEV void transform_pass_w(bool dst4, int shift, bool inverse, li16 *x)
{
  constexpr int L2 = W == 4 ? 2 : (W == 8 ? 3 : (W == 16 ? 4 : 5)), QN = 64 / W < 1 ? 1 : 64 / W, NOUT = W * W / 64 < 1 ? 1 : W * W / 64;
  const int add = 1 << (shift - 1), rs = dst4 ? 4 : 32 << (5 - L2);
  const KVZ_LDS int8_t *C = dst4 ? (const KVZ_LDS int8_t *)K->dst4 : (const KVZ_LDS int8_t *)K->dct32;
  IC_KEEP_DECL(out, NOUT, W * W);
  IC_FOR(tid) {
    const int j = tid & (W - 1), q = tid >> L2;
    if (tid < W * W) {
      int v[W];
      for (int i = 0; i < W; i++) v[i] = x[j * W + i];
      for (int t = 0; t < NOUT; t++) {
        const int m = q + QN * t;
        int acc = 0;
        if (!inverse) { for (int i = 0; i < W; i++) acc += (int)C[m * rs + i] * v[i]; }
        else { for (int i = 0; i < W; i++) acc += (int)C[i * rs + m] * v[i]; }
        acc = (acc + add) >> shift;
        IC_KEEP(out, t, m * W + j) = inverse ? iclip(-32768, 32767, acc) : (int)(i16)acc;
      }
    }
  }
  IC_SYNC();
  IC_FOR(tid) {
    const int j = tid & (W - 1), q = tid >> L2;
    if (tid < W * W) for (int t = 0; t < NOUT; t++) { const int m = q + QN * t; x[m * W + j] = (i16)IC_KEEP(out, t, m * W + j); }
  }
  IC_SYNC();
}
IC_DEV void transform_pass(bool dst4, int l2, int shift, bool inverse, li16 *x)
{
  if (l2 == 2) transform_pass_w<4>(dst4, shift, inverse, x);
  else if (l2 == 3) transform_pass_w<8>(false, shift, inverse, x);
  else if (l2 == 4) transform_pass_w<16>(false, shift, inverse, x);
  else transform_pass_w<32>(false, shift, inverse, x);
}
IC_FN bool quantize_tu(int lv, int c, int xl, int yl, int w, bool intra, bool early_skip)
{
  const int n = w * w;
  int l2 = 2;
  while ((1 << l2) < w) l2++;
  const bool dst = w == 4 && c == 0 && intra;
  const QScal qs = K->q[c ? 1 : 0][l2 - 2];
  const PView rv = lvl(lv, c, xl, yl), sv = orgv(c, xl, yl);
  gi16 *levels = coef(lv, c, xl, yl);
  li16 *tb = (li16 *)L->tb;
  // residual; the prediction stays where it is (the level's samples) until the reconstruction replaces it
  IC_FOR(tid) { for (int i = tid; i < n; i += KVZ_ICTU_THREADS) { const int yy = i >> l2, xx = i & (w - 1); tb[i] = (i16)((int)sv.p[yy * sv.s + xx] - (int)rv.p[yy * rv.s + xx]); } }
  IC_SYNC();
  transform_pass(dst, l2, l2 - 1, false, tb);
  transform_pass(dst, l2, l2 + 6, false, tb);
  // kvz_quant (quant-generic.c:68-81, no sign hiding) fused with "any level non-zero", kvz_fast_coeff_cost of the levels and -- into the TRANSPOSED position, for the
  // inverse passes -- kvz_dequant (quant-generic.c:298-340); all reads of the block before its writes.
  // Flat lists: one forward and one inverse factor for the block.  The LISTS builds (kvz_inter_ctu.hpp KVZ_ICTU_LISTS): the two factors of every position (kvz_recon.hpp
  // list_index, list_factor), from the plane of the block's list -- (intra CU ? 0 : 3) + c, list_plane_of; an intra CU of a B slice takes the intra lists under the
  // B slice's rounding -- in the picture's row at the block's QP, luma or chroma.  A picture without a set reads the flat list's row: the same path.
  u32 nz = 0, wsum = 0;
  const uint64_t weights = M->coeff_weights;
  IC_KEEP_DECL(deq, 16, 32 * 32);
#if KVZ_ICTU_LISTS_STATE
  QuantScalars dq;  // what dequant_product reads
  dq.dq_shift = qs.dq_shift; dq.dq_qp_per = qs.dq_qp_per;
  const KVZ_GLB u32 *plane = (c ? K->lf_c : K->lf_y) + list_plane_of(intra, c) * KVZ_LIST_PLANE;
#endif
  IC_FOR(tid) {
    // the factor words of the lane's whole trip (up to 16 at 32x32) leave together, ahead of the coefficient reads: HBM loads in flight behind one another and behind
    // the LDS reads, not one dependent load per coefficient
    u32 fw[16];
#if KVZ_ICTU_LISTS_STATE
    if (KVZ_ICTU_LISTS) {
#pragma unroll
      for (int t = 0; t < 16; t++) { const int i = tid + KVZ_ICTU_THREADS * t; fw[t] = i < n ? plane[list_index(l2, i)] : 0u; }
    }
#endif
    for (int t = 0; t < 16; t++) {
      const int i = tid + KVZ_ICTU_THREADS * t;
      if (i >= n) break;
      const int cf = tb[i];
      // 32 bits hold it: |cf| <= 2^15, a flat 8-bit list's multiplier <= 26214, add <= 171 << 18; with lists the multiplier is (26214 << 4) / 13 = 32263 at most
      // (entries >= 13: kvz_scaling_lists.hpp) and the product stays below 2^30 (kvz_recon.hpp quant_level) -- both operands within 24 bits either way
      const ListFactor lf = KVZ_ICTU_LISTS ? list_factor(fw[t]) : ListFactor{ qs.flat_q, 0 };
      int level = (int)((umul24((u32)iabs(cf), (u32)lf.fwd) + (u32)qs.add) >> qs.q_bits);
      if (cf < 0) level = -level;
      level = iclip(-32768, 32767, level);
      levels[i] = (i16)level;
      nz += level != 0;
      int a = iabs(level);
      if (a > 3) a = 3;
      wsum += (u32)((weights >> (16 * a)) & 0xffff);
#if KVZ_ICTU_LISTS_STATE
      // quant-generic.c:309-333, either side of its branch (dequant_product); |level| <= 2^15 and the inverse factor <= 72 * 255 fit the 24-bit multiply
      if (KVZ_ICTU_LISTS) IC_KEEP(deq, t, i) = dequant_product(mul24(level, lf.inv), dq);
      else
#endif
      IC_KEEP(deq, t, i) = iclip(-32768, 32767, (mul24(level, qs.dq_scale) + (1 << (qs.dq_shift - 1))) >> qs.dq_shift);
    }
  }
  const bool has = lanes_sum(nz) != 0;
  const u32 wtot = lanes_sum(wsum);
  L->ccost[c] = (double)wtot / 256.0;
  IC_SYNC();
  if (has && !early_skip) {
    IC_FOR(tid) { for (int t = 0; t < 16; t++) { const int i = tid + KVZ_ICTU_THREADS * t; if (i >= n) break; tb[(i & (w - 1)) * w + (i >> l2)] = (i16)IC_KEEP(deq, t, i); } }
    IC_SYNC();
    transform_pass(dst, l2, 7, true, tb);
    transform_pass(dst, l2, 12, true, tb);
    // residual (transposed storage) + prediction -> reconstruction
    IC_FOR(tid) { for (int i = tid; i < n; i += KVZ_ICTU_THREADS) { const int yy = i >> l2, xx = i & (w - 1); lu8 *r = rv.p + yy * rv.s + xx; *r = (u8)iclip(0, 255, (int)(i16)(tb[xx * w + yy] + (i16)*r)); } }
    IC_SYNC();
  }
  return has;
}

// ---- intra prediction in a B slice (oracle build_reference / intra_predict / rough_search) ----
// a reconstructed sample of plane c at picture position (px, py) that lies outside the CU under evaluation: the frame's reconstruction, where commit_down has put
// every finished CU of this CTU too
IC_DEV u8 rec_px(int c, int px, int py) { return recp(c)[py * (F.W >> (c ? 1 : 0)) + px]; }
// kvz_intra_build_reference_any (intra.c:305-425) into L->top / L->left, then the [1 2 1] smoothed copies in L->ftop / L->fleft: one reference sample per lane
// (entry i + 1 of either side: the i-th sample where it is available, the last available one past that -- intra.c:352-360, 400-408)
IC_FN void build_reference(int log2w, int c, int lx, int ly)
{
  const int sh = c ? 1 : 0, w = 1 << log2w;
  const int px = lx >> sh, py = ly >> sh, llx = lx & 63, lly = ly & 63;
  int avail_l = 0, avail_t = 0;
  if (lx > 0) {
    avail_l = K->avail_left[lly / 4][llx / 4] >> sh;
    if (avail_l > 2 * w) avail_l = 2 * w;
    if (avail_l > ((F.H - ly) >> sh)) avail_l = (F.H - ly) >> sh;
  }
  if (ly > 0) {
    avail_t = K->avail_top[lly / 4][llx / 4] >> sh;
    if (avail_t > 2 * w) avail_t = 2 * w;
    if (avail_t > ((F.W - lx) >> sh)) avail_t = (F.W - lx) >> sh;
  }
  IC_FOR(tid) {
    for (int i = tid; i < 4 * w + 1; i += KVZ_ICTU_THREADS) {
      if (i == 4 * w) {  // the corner
        const u8 corner = (lx > 0 && ly > 0) ? rec_px(c, px - 1, py - 1) : (lx > 0 ? rec_px(c, px - 1, py) : (ly > 0 ? rec_px(c, px, py - 1) : (u8)128));
        L->left[0] = L->top[0] = corner;  // without both neighbours: left[1], which is the nearest left sample, the sample above, or 128
      } else if (i < 2 * w) {  // left[i + 1]
        u8 v;
        if (lx > 0) v = rec_px(c, px - 1, py + (i < avail_l ? i : avail_l - 1));
        else v = ly > 0 ? rec_px(c, px, py - 1) : (u8)128;
        L->left[i + 1] = v;
      } else {  // top[j + 1]
        const int j = i - 2 * w;
        u8 v;
        if (ly > 0) v = rec_px(c, px + (j < avail_t ? j : avail_t - 1), py - 1);
        else v = lx > 0 ? rec_px(c, px - 1, py) : (u8)128;
        L->top[j + 1] = v;
      }
    }
  }
  IC_SYNC();
  IC_FOR(tid) {  // intra_filter_reference (intra.c:176-204)
    const int n = 2 * w + 1;
    const u8 *top = L->top, *left = L->left;
    for (int i = tid; i < n; i += KVZ_ICTU_THREADS) {
      if (i == 0) L->fleft[0] = L->ftop[0] = (u8)((left[1] + 2 * left[0] + top[1] + 2) / 4);
      else if (i == n - 1) { L->fleft[n - 1] = left[n - 1]; L->ftop[n - 1] = top[n - 1]; }
      else { L->fleft[i] = (u8)((left[i - 1] + 2 * left[i] + left[i + 1] + 2) / 4); L->ftop[i] = (u8)((top[i - 1] + 2 * top[i] + top[i + 1] + 2) / 4); }
    }
  }
  IC_SYNC();
}
// Value of angular mode `mode` at pixel (x, y) (intra-generic.c:49-155; kvz_ops.hpp angular_pixel with its two tables as constants in the instruction stream -- a local
// array indexed at run time lives in memory): sample_disp {0,2,5,9,13,17,21,26,32} six bits each, the inverse angles {-,4096,1638,910,630,482,390,315,256} a select chain
IC_DEV u8 angular_px(int mode, int x, int y, const u8 *above, const u8 *left)
{
  const bool vertical = mode >= 18;
  const int mode_disp = vertical ? mode - 26 : 10 - mode;
  const int ad = iabs(mode_disp);
  const unsigned long long disp_tab = 0ull | 2ull << 6 | 5ull << 12 | 9ull << 18 | 13ull << 24 | 17ull << 30 | 21ull << 36 | 26ull << 42 | 32ull << 48;
  const int disp = (int)((disp_tab >> (6 * ad)) & 63ull);
  const int sample_disp = mode_disp < 0 ? -disp : disp;
  const u8 *main_ref = vertical ? above : left, *side_ref = vertical ? left : above;
  const int px = vertical ? x : y, py = vertical ? y : x;  // horizontal modes = vertical on swapped refs, transposed
  if (sample_disp == 0) return main_ref[px + 1];
  const int delta_pos = (py + 1) * sample_disp;
  const int di = delta_pos >> 5, df = delta_pos & 31;
  const int inv = ad == 1 ? 4096 : (ad == 2 ? 1638 : (ad == 3 ? 910 : (ad == 4 ? 630 : (ad == 5 ? 482 : (ad == 6 ? 390 : (ad == 7 ? 315 : 256))))));
  const int r1 = angular_ref(main_ref, side_ref, px + di, inv);
  if (!df) return (u8)r1;
  const int r2 = angular_ref(main_ref, side_ref, px + di + 1, inv);
  return (u8)(((32 - df) * r1 + df * r2 + 16) >> 5);
}
// kvz_intra_predict (intra.c:252-301) of one sample
IC_DEV u8 intra_pixel(int log2w, int mode, int c, int x, int y)
{
  const int w = 1 << log2w;
  bool filtered = false;
  if (c != 0 || mode == 1 || w == 4) filtered = false;
  else if (mode == 0) filtered = true;
  else {
    const int thres = log2w == 3 ? 7 : (log2w == 4 ? 1 : 0);  // intra.c:262-281 { 0, 7, 1, 0, 0 }[log2w - 2]
    const int d26 = iabs(mode - 26), d10 = iabs(mode - 10);
    if ((d26 < d10 ? d26 : d10) > thres) filtered = true;
  }
  const u8 *ut = filtered ? L->ftop : L->top, *ul = filtered ? L->fleft : L->left;
  if (mode == 0) return planar_pixel(log2w, x, y, ut, ul);
  if (mode == 1) {
    const int dc = dc_value(log2w, ut, ul);
    return (c == 0 && w < 32) ? filtered_dc_pixel(dc, x, y, ut, ul) : (u8)dc;
  }
  u8 v = angular_px(mode, x, y, ut, ul);
  if (c == 0 && w < 32 && ((mode == 26 && x == 0) || (mode == 10 && y == 0))) {  // intra_post_process_angular (intra.c:207-219)
    const u8 *ref = mode == 10 ? ut : ul;
    const int i = mode == 10 ? x : y;
    v = clip_pixel((int)v + (((int)ref[i + 1] - (int)ref[0]) >> 1));
  }
  return v;
}
// ---- all 35 intra modes of a CU scored at once (search_intra.c:391-530 visits 13-18 of them in 3-4 dependent rounds; every score is a pure function of (references,
// source), so the selection is replayed on the full table): the design of the all-intra pass (kvz_ctu.hpp angular_block_satd / rough_search) on this pass's LDS block ----
// signed sample displacement of angular mode m (intra-generic.c:59-60, 70-76): {0,2,5,9,13,17,21,26,32}[|d|], d = m - 26 (vertical, m >= 18) or 10 - m
IC_DEV int mode_disp_of(int mode)
{
  const int md = mode >= 18 ? mode - 26 : 10 - mode, ad = iabs(md);
  const unsigned long long disp_tab = 0ull | 2ull << 6 | 5ull << 12 | 9ull << 18 | 13ull << 24 | 17ull << 30 | 21ull << 36 | 26ull << 42 | 32ull << 48;
  const int disp = (int)((disp_tab >> (6 * ad)) & 63ull);
  return md < 0 ? -disp : disp;
}
IC_DEV int mode_inv_of(int mode)
{
  const int ad = iabs(mode >= 18 ? mode - 26 : 10 - mode);
  return ad == 1 ? 4096 : (ad == 2 ? 1638 : (ad == 3 ? 910 : (ad == 4 ? 630 : (ad == 5 ? 482 : (ad == 6 ? 390 : (ad == 7 ? 315 : 256))))));
}
#ifdef KVZ_HOSTSIM
struct IcPk { i16 lo, hi; };
IC_DEV IcPk ipk(int lo, int hi) { IcPk r = { (i16)lo, (i16)hi }; return r; }
IC_DEV IcPk ipk_add(IcPk a, IcPk b) { return ipk(a.lo + b.lo, a.hi + b.hi); }
IC_DEV IcPk ipk_sub(IcPk a, IcPk b) { return ipk(a.lo - b.lo, a.hi - b.hi); }
IC_DEV u32 ipk_absmax(IcPk a) { return (u32)imax(iabs(a.lo), iabs(a.hi)); }
#else
typedef ic_pk16 IcPk;
IC_DEV IcPk ipk(int lo, int hi) { return pk_from(lo, hi); }
IC_DEV IcPk ipk_add(IcPk a, IcPk b) { return a + b; }
IC_DEV IcPk ipk_sub(IcPk a, IcPk b) { return a - b; }
IC_DEV u32 ipk_absmax(IcPk a) { return pk_absmax2(a); }
#endif
// One angular mode (2 .. 33) on one 8x8 block (bx, by) of the w x w CU at LCU position (xl, yl), predicted from the references in LDS and Hadamard-scored without leaving
// registers: the block's sum |H D H^T| of picture-generic.c:252-340 (before the (s + 2) >> 2 rounding), D = intra-generic.c:49-155 prediction minus source.  Horizontal
// modes run on the transposed problem (main reference = left, source block transposed: the Hadamard magnitudes of D^T are those of D).  PAIR (device): the block is
// shared by two neighbouring lanes, `half` 0 / 1 taking rows 0..3 / 4..7 across the main reference; they swap for the butterfly stage that pairs row r with row r + 4
// (DPP quad_perm) and both return the block's total.
template <bool PAIR> IC_DEV u32 angular_block_satd(int log2w, int mode, int bx, int by, int xl, int yl, int half)
{
  const int w = 1 << log2w;
  const bool vertical = mode >= 18;
  const int disp = mode_disp_of(mode);
  const int p0 = vertical ? bx : by, q0 = vertical ? by : bx;  // block origin along / across the main reference
  const bool filt = imin(iabs(mode - 26), iabs(mode - 10)) > (log2w == 3 ? 7 : (log2w == 4 ? 1 : 0));
  const lu8 *mr;
  if (disp < 0) mr = (const lu8 *)L->mref[mode - 11] + IC_MREF_ORG;
  else mr = filt ? (vertical ? (const lu8 *)L->ftop : (const lu8 *)L->fleft) : (vertical ? (const lu8 *)L->top : (const lu8 *)L->left);
  mr += p0 + 1;
  const PView ov = orgv(0, xl + bx, yl + by);
  const lu8 *org = vertical ? ov.p : (const lu8 *)L->org_t + bx * w + by;
  const int ostride = vertical ? ov.s : w;
  const lu8 *side = vertical ? (const lu8 *)L->left : (const lu8 *)L->top;  // intra.c:207-219: modes 10 / 26 add the gradient of the unfiltered side reference to their first line
  const bool edge = disp == 0 && p0 == 0;
  constexpr int NR = PAIR ? 4 : 8;
  const int r0 = PAIR ? 4 * half : 0;
  IcPk d[NR][4];
  for (int i = 0; i < NR; i++) {
    const int r = r0 + i;
    const int qa = q0 + r + 1, delta = qa * disp, di = delta >> 5, df = delta & 31;
    const lu8 *m = mr + di;
    const unsigned long long ow = lds_read64(org + r * ostride);  // block origins are multiples of 8 in 8-byte aligned arrays
    int v[8];
    int a = m[0];
    for (int k = 0; k < 8; k++) {
      const int b = m[k + 1];
      v[k] = ((32 - df) * a + df * b + 16) >> 5;
      a = b;
    }
    if (edge) v[0] = iclip(0, 255, v[0] + (((int)side[qa] - (int)side[0]) >> 1));
    for (int j = 0; j < 4; j++) d[i][j] = ipk(v[2 * j] - (int)((ow >> (16 * j)) & 0xff), v[2 * j + 1] - (int)((ow >> (16 * j + 8)) & 0xff));
  }
  for (int i = 0; i < NR; i++) {  // along the rows: columns k and k + 4, then k and k + 2 (k and k + 1 is the folded stage)
    const IcPk a0 = ipk_add(d[i][0], d[i][2]), a1 = ipk_add(d[i][1], d[i][3]), a2 = ipk_sub(d[i][0], d[i][2]), a3 = ipk_sub(d[i][1], d[i][3]);
    d[i][0] = ipk_add(a0, a1); d[i][1] = ipk_sub(a0, a1); d[i][2] = ipk_add(a2, a3); d[i][3] = ipk_sub(a2, a3);
  }
  u32 sum = 0;
  if constexpr (PAIR) {
#ifndef KVZ_HOSTSIM
    for (int j = 0; j < 4; j++) {  // down the columns, two columns per register
      IcPk e[4];
      for (int i = 0; i < 4; i++) {  // rows r and r + 4 live in the two lanes of the pair
        const IcPk o = pk_dpp<0xB1 /* quad_perm [1,0,3,2] */, 0xF>(d[i][j], d[i][j]);
        e[i] = half ? ipk_sub(o, d[i][j]) : ipk_add(d[i][j], o);
      }
      const IcPk b0 = ipk_add(e[0], e[2]), b1 = ipk_add(e[1], e[3]), b2 = ipk_sub(e[0], e[2]), b3 = ipk_sub(e[1], e[3]);
      sum += ipk_absmax(ipk_add(b0, b1)) + ipk_absmax(ipk_sub(b0, b1)) + ipk_absmax(ipk_add(b2, b3)) + ipk_absmax(ipk_sub(b2, b3));
    }
    sum += (u32)__builtin_amdgcn_update_dpp(0, (int)sum, 0xB1, 0xF, 0xF, false);
#endif
  } else {
    for (int j = 0; j < 4; j++) {  // down the columns, two columns per register
      const IcPk a0 = ipk_add(d[0][j], d[4 % NR][j]), a1 = ipk_add(d[1][j], d[5 % NR][j]), a2 = ipk_add(d[2][j], d[6 % NR][j]), a3 = ipk_add(d[3][j], d[7 % NR][j]);
      const IcPk a4 = ipk_sub(d[0][j], d[4 % NR][j]), a5 = ipk_sub(d[1][j], d[5 % NR][j]), a6 = ipk_sub(d[2][j], d[6 % NR][j]), a7 = ipk_sub(d[3][j], d[7 % NR][j]);
      const IcPk b0 = ipk_add(a0, a2), b1 = ipk_add(a1, a3), b2 = ipk_sub(a0, a2), b3 = ipk_sub(a1, a3);
      const IcPk b4 = ipk_add(a4, a6), b5 = ipk_add(a5, a7), b6 = ipk_sub(a4, a6), b7 = ipk_sub(a5, a7);
      sum += ipk_absmax(ipk_add(b0, b1)) + ipk_absmax(ipk_sub(b0, b1)) + ipk_absmax(ipk_add(b2, b3)) + ipk_absmax(ipk_sub(b2, b3));
      sum += ipk_absmax(ipk_add(b4, b5)) + ipk_absmax(ipk_sub(b4, b5)) + ipk_absmax(ipk_add(b6, b7)) + ipk_absmax(ipk_sub(b6, b7));
    }
  }
  return 2 * sum;
}
// SATD (satd_NxN: 8x8 Hadamard tiles, each (sum + 2) >> 2) of ALL 35 modes' predictions of the luma block at (xl, yl) (from the references build_reference left in LDS) into
// L->mcost[mode].  Phase 1: the extended main references of the modes with negative displacement, the transposed source block, the predictions of planar, DC and mode
// 34 as LDS planes (33 angular modes x 2 lanes would not fill whole wavefronts).  Phase 2: modes 2 .. 33 in registers, two lanes per (mode, 8x8 block); the three planes through satd_tiles.
IC_FN void intra_all_mode_costs(int log2w, int xl, int yl)
{
  const int w = 1 << log2w, nblk = (w >> 3) * (w >> 3), lb = 2 * (log2w - 3);
  const int thres = log2w == 3 ? 7 : (log2w == 4 ? 1 : 0), nq = 2 * w + 2;
  const PView so = orgv(0, xl, yl);
  IC_FOR(tid) {
    for (int i = tid; i < 15 * nq; i += KVZ_ICTU_THREADS) {
      const int mi = i / nq, mode = 11 + mi, q = i - mi * nq - w;
      const bool vertical = mode >= 18, filt = imin(iabs(mode - 26), iabs(mode - 10)) > thres;
      const u8 *top = filt ? L->ftop : L->top, *left = filt ? L->fleft : L->left;
      const u8 *main_ref = vertical ? top : left, *side_ref = vertical ? left : top;
      const int idx = q >= 0 ? q : (128 + (-q) * mode_inv_of(mode)) >> 8;
      L->mref[mi][IC_MREF_ORG + q] = (q >= 0 ? main_ref : side_ref)[imin(idx, 2 * w)];
    }
    for (int e = tid; e < w * w; e += KVZ_ICTU_THREADS) { const int ex = e >> log2w, ey = e & (w - 1); L->org_t[e] = so.p[ey * so.s + ex]; }
    for (int i = tid; i < 3 * w * w; i += KVZ_ICTU_THREADS) {
      const int mi = i >> (2 * log2w), e = i & (w * w - 1);
      L->flat[mi][e] = intra_pixel(log2w, mi == 2 ? 34 : mi, 0, e & (w - 1), e >> log2w);
    }
    for (int v = tid; v < 35; v += KVZ_ICTU_THREADS) L->mcost[v] = 0;
  }
  IC_SYNC();
  IC_FOR(tid) {
#ifdef KVZ_HOSTSIM
    for (int t = tid; t < 32 * nblk; t += KVZ_ICTU_THREADS) {  // one "lane" per (mode, block)
      const int mode = 2 + (t >> lb), b = t & (nblk - 1), bx = (b & ((w >> 3) - 1)) * 8, by = (b >> (log2w - 3)) * 8;
      IC_LDS_ADD(&L->mcost[mode], (angular_block_satd<false>(log2w, mode, bx, by, xl, yl, 0) + 2) >> 2);
    }
#else
    for (int t = tid; t < 64 * nblk; t += KVZ_ICTU_THREADS) {  // 64 lane tasks for an 8x8 CU, 256 for a 16x16 one: whole wavefronts
      const int p = t >> 1, mode = 2 + (p >> lb), b = p & (nblk - 1), bx = (b & ((w >> 3) - 1)) * 8, by = (b >> (log2w - 3)) * 8;
      const u32 v = angular_block_satd<true>(log2w, mode, bx, by, xl, yl, t & 1);
      if (!(t & 1)) IC_LDS_ADD(&L->mcost[mode], (v + 2) >> 2);
    }
#endif
  }
  satd_tiles(3 * nblk, w, so.s,
             [=](int it, const lu8 *&pa, const lu8 *&pb) {
               const int mi = it >> lb, b = it & (nblk - 1), bx = (b & ((w >> 3) - 1)) * 8, by = (b >> (log2w - 3)) * 8;
               pa = (const lu8 *)L->flat[mi] + by * w + bx; pb = so.p + by * so.s + bx;
             },
             [=](int it, u32 v) { const int mi = it >> lb; IC_LDS_ADD(&L->mcost[mi == 2 ? 34 : mi], v); });
  IC_SYNC();
  IC_FOR(tid) { if (tid == 0) L->intra_done = ~0ull; }
  IC_SYNC();
}

// SATD (satd_NxN: 8x8 Hadamard tiles) of the predictions of the intra modes in `want` that L->intra_done does not hold yet (from the references in LDS) against the source
// block at (xl, yl) into L->mcost[mode].  kvazaar scores its modes one pair at a time (search_intra.c:433-519); every score is a pure function of (references, source),
// so the caller asks for everything a step of the selection can need at once -- the coarse grid together with the most probable modes, planar and DC, then the two
// neighbours of each refinement step -- and replays the selection on the table.  Two phases: the predictions into LDS planes (the mode is uniform inside a phase), then
// one item per (mode, 8x8 tile).
IC_FN void intra_mode_costs(int log2w, int xl, int yl, unsigned long long want)
{
  const int w = 1 << log2w, ww = w * w, tw = w >> 3, tiles = tw * tw;
  unsigned long long todo = want & ~L->intra_done;
  if (!todo) return;
  L->intra_done |= todo;
  lu8 *planes = (lu8 *)L->planes;
  const int room = (int)sizeof(L->planes) / ww;  // predictions scored per round: eight 16x16 blocks, thirty-two 8x8
  const PView so = orgv(0, xl, yl);
  while (todo) {
    int n = 0;
    for (int mode = 0; mode < 35 && n < room; mode++) {
      if (!((todo >> mode) & 1)) continue;
      todo &= ~(1ull << mode);
      L->todo[n] = (int8_t)mode;
      L->mcost[mode] = 0;
      IC_FOR(tid) { for (int i = tid; i < ww; i += KVZ_ICTU_THREADS) planes[n * ww + i] = intra_pixel(log2w, mode, 0, i & (w - 1), i >> log2w); }
      n++;
    }
    IC_SYNC();
    satd_tiles(n * tiles, w, so.s,
               [=](int it, const lu8 *&pa, const lu8 *&pb) {
                 const int slot = it >> (2 * (log2w - 3)), t = it & (tiles - 1), ty = t >> (log2w - 3), tx = t & (tw - 1);
                 pa = planes + slot * ww + ty * 8 * w + tx * 8; pb = so.p + ty * 8 * so.s + tx * 8;
               },
               [=](int it, u32 v) { IC_LDS_ADD(&L->mcost[L->todo[it >> (2 * (log2w - 3))]], v); });
    IC_SYNC();
  }
}
