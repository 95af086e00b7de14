// kvz_inter_ctu_cand.inc -- part of struct InterCtu (kvz_inter_ctu.hpp): merge and AMVP candidate derivation (inter.c:686-1572), scalar code every lane runs alike.

IC_DEV bool a0_coded(int x, int y, int width, int height)
{
  int size = (width & -width) < (height & -height) ? (width & -width) : (height & -height);
  if (height != size) y = y + height - size;
  while (size < 64) {
    const int parent = 2 * size, idx = ((x & (parent - 1)) != 0) + 2 * ((y & (parent - 1)) != 0);  // (powers of two, non-negative positions)
    if (idx == 0) return true;
    if (idx == 1 || idx == 3) return false;
    y -= size; size = parent;
  }
  return false;
}
IC_DEV bool b0_coded(int x, int y, int width, int height)
{
  int size = (width & -width) < (height & -height) ? (width & -width) : (height & -height);
  if (width != size) x = x + width - size;
  while (size < 64) {
    const int parent = 2 * size, idx = ((x & (parent - 1)) != 0) + 2 * ((y & (parent - 1)) != 0);  // (powers of two, non-negative positions)
    if (idx == 0 || idx == 2) return true;
    if (idx == 3) return false;
    x -= size; size = parent;
  }
  return true;
}

// A candidate's motion, packed: what the derivation works on, in registers.  The seven candidates' records are fetched by seven LANES at once (one round trip to the
// decided picture's records in LDS / to the frame's in HBM for all of them) and handed to every lane as wavefront-uniform values; the rest is scalar code on registers.
// (Round 5 kept the records in LDS and read them back field by field: chains of dependent LDS round trips, 15 % of the pass.)
struct Mot { u32 m0, m1, d; };  // mv[0], mv[1] as x | y << 16;  d = mv_dir | mv_ref[0] << 8 | mv_ref[1] << 16 | (a usable candidate: there, inter) << 24
IC_DEV Mot mot_of(const CuInfo &c)
{
  Mot m;
  m.m0 = (u32)(uint16_t)c.mv[0][0] | (u32)(uint16_t)c.mv[0][1] << 16;
  m.m1 = (u32)(uint16_t)c.mv[1][0] | (u32)(uint16_t)c.mv[1][1] << 16;
  m.d = (u32)c.mv_dir | (u32)c.mv_ref[0] << 8 | (u32)c.mv_ref[1] << 16 | (c.type == 2 ? 1u << 24 : 0u);
  return m;
}
IC_DEV bool mot_valid(const Mot &m) { return (m.d >> 24) != 0; }
// candidate i of the PU: 0 a0, 1 a1, 2 b0, 3 b1, 4 b2 (get_spatial_merge_candidates, inter.c:869-945), 5 the temporal bottom-right one, 6 the temporal centre
// (get_temporal_merge_candidates, inter.c:766-855: the reference FRAME's records at the picture-LOCAL position, checked against the frame's size -- inter.c:836-905 is
// handed the tile's x, y and compares with encoder_control->in.width / height; for a picture that is the frame there is no difference)
IC_DEV Mot cand_fetch(int i, int x, int y, int w, int h, bool a0c, bool b0c, bool tmvp)
{
  const Mot none = { 0u, 0u, 0u };
  if (i < 5) {
    const int xl = x - cx, yl = y - cy;
    const int px = i == 2 ? x + w : (i == 3 ? x + w - 1 : x - 1), py = i == 0 ? y + h : (i == 1 ? y + h - 1 : y - 1);
    const bool left = x != 0, above = y != 0;
    const bool ok = i == 0 ? (left && yl + h < 64 && y + h < F.H && a0c) : i == 1 ? left : i == 2 ? (above && x + w < F.W && (xl + w < 64 || yl == 0) && b0c) : i == 3 ? above : (above && left);
    if (!ok) return none;
    return mot_of(cell_at(px, py));
  }
  const int px = i == 5 ? x + w : x + w / 2, py = i == 5 ? y + h : y + h / 2;
  if (!(tmvp && px < K->ref_w && py < K->ref_h && (i != 5 || (py & 63) != 0))) return none;
  return mot_of(load_cu((const CuInfo *)((const uint8_t *)ref_cu_frame() + mul24(((px >> 4) << 2) + mul24((py >> 4) << 2, K->ref_w >> 2), (int)sizeof(CuInfo)))));
}
struct Cands { Mot a0, a1, b0, b1, b2, th, tc; };  // (named, not an array: an array the compiler indexes lives in scratch memory)
IC_DEV Mot mot_sel(bool c, const Mot &a, const Mot &b) { return Mot{ c ? a.m0 : b.m0, c ? a.m1 : b.m1, c ? a.d : b.d }; }
IC_DEV Mot mot_lane(const Mot &mine, int i)  // lane i's value, to every lane
{
#ifdef KVZ_HOSTSIM
  (void)i; return mine;
#else
  return Mot{ (u32)__builtin_amdgcn_readlane((int)mine.m0, i), (u32)__builtin_amdgcn_readlane((int)mine.m1, i), (u32)__builtin_amdgcn_readlane((int)mine.d, i) };
#endif
}
IC_DEV Cands cand_gather(int x, int y, int w, int h)
{
  IC_COUNT(18);
  const bool a0c = a0_coded(x, y, w, h), b0c = b0_coded(x, y, w, h), tmvp = !(M->poc < 1 || M->no_tmvp);
  Cands c;
#ifdef KVZ_HOSTSIM
  c.a0 = cand_fetch(0, x, y, w, h, a0c, b0c, tmvp); c.a1 = cand_fetch(1, x, y, w, h, a0c, b0c, tmvp); c.b0 = cand_fetch(2, x, y, w, h, a0c, b0c, tmvp); c.b1 = cand_fetch(3, x, y, w, h, a0c, b0c, tmvp);
  c.b2 = cand_fetch(4, x, y, w, h, a0c, b0c, tmvp); c.th = cand_fetch(5, x, y, w, h, a0c, b0c, tmvp); c.tc = cand_fetch(6, x, y, w, h, a0c, b0c, tmvp);
#else
  Mot mine = { 0u, 0u, 0u };
  const int lane = (int)(threadIdx.x & 63u);  // (every wavefront of the workgroup for itself)
  if (lane < 7) mine = cand_fetch(lane, x, y, w, h, a0c, b0c, tmvp);
  c.a0 = mot_lane(mine, 0); c.a1 = mot_lane(mine, 1); c.b0 = mot_lane(mine, 2); c.b1 = mot_lane(mine, 3); c.b2 = mot_lane(mine, 4); c.th = mot_lane(mine, 5); c.tc = mot_lane(mine, 6);
#endif
  return c;
}
// the motion one list of a temporal candidate predicts (inter.c:1093-1135 with one reference picture: the co-located vector of that list, else of the other)
IC_DEV u32 temporal_mv(const Mot &col, int reflist) { return reflist ? ((col.d & 2u) ? col.m1 : col.m0) : ((col.d & 1u) ? col.m0 : col.m1); }
// ... and, in a launch with reference lists, scaled to entry r of the picture's list from the co-located picture -- entry 0 -- and the picture ITS vector
// referred to (add_temporal_candidate, inter.c:1134-1184; a P record moves by list 0)
IC_DEV u32 temporal_mv_to(const Mot &col, int r)
{
#if KVZ_ICTU_REFS_STATE
  if (KVZ_ICTU_REFS) {
    const int scale = L->rf.temporal[r & 3][(col.d >> ((col.d & 1u) ? 8 : 16)) & 3u];
    if (scale != KVZ_MV_SCALE_NONE) IC_REFS_EVENT(1);
    return mv_scale_packed(temporal_mv(col, 0), scale);
  }
#endif
  return temporal_mv(col, 0);
}
IC_DEV bool same_motion(const Mot &a, const Mot &b)  // b is there and moves as a does
{
  if (!mot_valid(b)) return false;
  const u32 x = a.d ^ b.d;
  if (x & 0xffu) return false;
  if ((a.d & 1u) && (a.m0 != b.m0 || (x & 0xff00u))) return false;
  if ((a.d & 2u) && (a.m1 != b.m1 || (x & 0xff0000u))) return false;
  return true;
}
struct Mot5 { Mot e0, e1, e2, e3, e4; };
IC_DEV void mot_put(Mot5 &e, int n, const Mot &v)  // e[n] = v
{
  e.e0 = mot_sel(n == 0, v, e.e0); e.e1 = mot_sel(n == 1, v, e.e1); e.e2 = mot_sel(n == 2, v, e.e2); e.e3 = mot_sel(n == 3, v, e.e3); e.e4 = mot_sel(n == 4, v, e.e4);
}
IC_DEV Mot mot_at(const Mot5 &e, int i) { return i == 0 ? e.e0 : (i == 1 ? e.e1 : (i == 2 ? e.e2 : (i == 3 ? e.e3 : e.e4))); }  // (i a constant where it is used)
static_assert(sizeof(MCand) == 12, "a merge candidate is written as three words: mv[0], mv[1], ref[0] | ref[1] << 8 | dir << 16");

// inter.c:1440-1572 kvz_inter_get_merge_cand, B slice -- or, KVZ_ICTU_P, P slice -- with one reference picture
// into L->pu.merge
IC_FN int merge_candidates(int x, int y, int w, int h)
{
  const int max = 5;
  int n = 0;
  const Cands c = cand_gather(x, y, w, h);
  const Mot zero = { 0u, 0u, 0u };
  Mot5 e = { zero, zero, zero, zero, zero };
  if (mot_valid(c.a1)) { mot_put(e, n, Mot{ c.a1.m0, c.a1.m1, c.a1.d & 0xffffffu }); n++; }
  if (mot_valid(c.b1) && !same_motion(c.b1, c.a1)) { mot_put(e, n, Mot{ c.b1.m0, c.b1.m1, c.b1.d & 0xffffffu }); n++; }
  if (mot_valid(c.b0) && !same_motion(c.b0, c.b1)) { mot_put(e, n, Mot{ c.b0.m0, c.b0.m1, c.b0.d & 0xffffffu }); n++; }
  if (mot_valid(c.a0) && !same_motion(c.a0, c.a1)) { mot_put(e, n, Mot{ c.a0.m0, c.a0.m1, c.a0.d & 0xffffffu }); n++; }
  if (n < 4 && mot_valid(c.b2) && !same_motion(c.b2, c.a1) && !same_motion(c.b2, c.b1)) { mot_put(e, n, Mot{ c.b2.m0, c.b2.m1, c.b2.d & 0xffffffu }); n++; }
  const int n_spatial = n;
  if (n < max && (mot_valid(c.th) || mot_valid(c.tc))) {
    const Mot col = mot_sel(mot_valid(c.th), c.th, c.tc);
    if (KVZ_ICTU_P) mot_put(e, n, Mot{ temporal_mv_to(col, 0), 0u, 1u });  // inter.c:1479 max_reflist 0 in a P slice: list 0 only, reference index 0 (:1490-1496)
    else mot_put(e, n, Mot{ temporal_mv(col, 0), temporal_mv(col, 1), 3u });
    n++;
  }
  const int n_temporal = n;
  if (!KVZ_ICTU_P && n < max) {  // (inter.c:1504: combined bi-predictive candidates are a B slice's)
    // the pairs (0,1) (1,0) (0,2) (2,0) (1,2) (2,1) (0,3) (3,0) (1,3) (3,1) (2,3) (3,2) of inter.c:1518-1519, unrolled: every entry named by a constant
    const int pairs = n * (n - 1);
    bool go = true;
#pragma unroll
    for (int idx = 0; idx < 12; idx++) {
      const int i = (int)((0xedc984u >> (2 * idx)) & 3u), j = (int)((0xb73621u >> (2 * idx)) & 3u);
      if (go && !(idx < pairs && n != max)) go = false;
      if (go && (i >= n || j >= n)) go = false;
      const Mot ei = mot_at(e, i), ej = mot_at(e, j);
      if (go && (ei.d & 1u) && (ej.d & 2u) && ei.m0 != ej.m1) {  // (the reference writes an entry it then does not count; the next one or the filling below writes it again)
        mot_put(e, n, Mot{ ei.m0, ej.m1, 3u | (ei.d & 0xff00u) | (ej.d & 0xff0000u) });
        n++;
      }
    }
  }
  IC_MERGE_ORIGIN(x, y, w, n_spatial, n_temporal, n);  // (the host simulation's census: entries below n_spatial are neighbours', then the temporal one, from n on zero)
  const Mot fill = { 0u, 0u, KVZ_ICTU_P ? 1u : 3u };  // inter.c:1556-1569: the zero candidates, dir 1 in a P slice
#if KVZ_ICTU_REFS_STATE
  if (KVZ_ICTU_REFS) {  // inter.c:1539-1569 with num_ref the length of the list: zero candidate z refers to entry z while z < num_ref - 1, to entry 0 from there on (ref[1] = ref[0])
    const int nr = list_length();
    auto zero_of = [&](int k) { const u32 r = (k - n >= nr - 1 || k < n) ? 0u : (u32)(k - n); return Mot{ 0u, 0u, 1u | r << 8 | r << 16 }; };
    e.e0 = mot_sel(n <= 0, zero_of(0), e.e0); e.e1 = mot_sel(n <= 1, zero_of(1), e.e1); e.e2 = mot_sel(n <= 2, zero_of(2), e.e2); e.e3 = mot_sel(n <= 3, zero_of(3), e.e3); e.e4 = mot_sel(n <= 4, zero_of(4), e.e4);
#ifdef KVZ_HOSTSIM
    L->pu.zero_from = n;
#endif
  } else
#endif
  { e.e0 = mot_sel(n <= 0, fill, e.e0); e.e1 = mot_sel(n <= 1, fill, e.e1); e.e2 = mot_sel(n <= 2, fill, e.e2); e.e3 = mot_sel(n <= 3, fill, e.e3); e.e4 = mot_sel(n <= 4, fill, e.e4); }
  // which entries repeat an earlier one (the merge analysis skips them, search_inter.c:1710-1730: it compares with the entries it kept -- an earlier equal entry was
  // kept, or was skipped for what skips this one too)
  // (In a P slice too the reference compares the fields of list 1, which move no sample: a neighbour's record carries mv_ref[1] 255 from the search and 0 from a
  // temporal or zero candidate it merged with, and an entry that repeats an earlier one's list-0 motion under another mv_ref[1] is evaluated, and can be the
  // cheaper one to signal.  What inter.c:1476-1569 does not write of such an entry in a P slice -- mv[1], and ref[1] of the temporal one -- is zero here)
  auto same = [](const Mot &a, const Mot &b) { return a.m0 == b.m0 && a.m1 == b.m1 && a.d == b.d; };
  int dup = 0;
  if (same(e.e1, e.e0)) dup |= 2;
  if (same(e.e2, e.e0) || same(e.e2, e.e1)) dup |= 4;
  if (same(e.e3, e.e0) || same(e.e3, e.e1) || same(e.e3, e.e2)) dup |= 8;
  if (same(e.e4, e.e0) || same(e.e4, e.e1) || same(e.e4, e.e2) || same(e.e4, e.e3)) dup |= 16;
  L->pu.merge_dup = dup;
  MCand *out = L->pu.merge;
#ifdef KVZ_HOSTSIM
  for (int k = 0; k < 5; k++) {
    const Mot ek = mot_at(e, k);
    out[k].mv[0][0] = (i16)(ek.m0 & 0xffffu); out[k].mv[0][1] = (i16)(ek.m0 >> 16); out[k].mv[1][0] = (i16)(ek.m1 & 0xffffu); out[k].mv[1][1] = (i16)(ek.m1 >> 16);
    out[k].ref[0] = (u8)(ek.d >> 8); out[k].ref[1] = (u8)(ek.d >> 16); out[k].dir = (u8)ek.d;
  }
#else
  u32 v = 0;  // word t of the list in lane t  (v_writelane: the lane as a constant -- two scalar registers in one VOP3 are one too many)
#define IC_PUT_ENTRY(k, ek) do { const u32 refs_dir_ = (((ek).d >> 8) & 0xffffu) | ((ek).d & 0xffu) << 16; \
    asm("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(__builtin_amdgcn_readfirstlane((int)(ek).m0)), "n"(3 * (k))); asm("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(__builtin_amdgcn_readfirstlane((int)(ek).m1)), "n"(3 * (k) + 1)); \
    asm("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(__builtin_amdgcn_readfirstlane((int)refs_dir_)), "n"(3 * (k) + 2)); } while (0)
  IC_PUT_ENTRY(0, e.e0); IC_PUT_ENTRY(1, e.e1); IC_PUT_ENTRY(2, e.e2); IC_PUT_ENTRY(3, e.e3); IC_PUT_ENTRY(4, e.e4);
#undef IC_PUT_ENTRY
  if ((threadIdx.x & 63u) < 15u) ((KVZ_LDS u32 *)out)[threadIdx.x & 63u] = v;
#endif
  return max;
}

IC_DEV bool add_mvp(const Mot &cand, int reflist, u32 &mv)  // the candidate's vector of the list, else of the other list (one reference picture: no scaling)
{
  if (!mot_valid(cand)) return false;
  const u32 first = reflist ? 2u : 1u, second = reflist ? 1u : 2u;
  if (cand.d & first) { mv = reflist ? cand.m1 : cand.m0; return true; }
  if (!KVZ_ICTU_P && (cand.d & second)) { mv = reflist ? cand.m0 : cand.m1; return true; }  // (no record of a P picture or of its reference moves by list 1)
  return false;
}
IC_DEV void store_mv32(i16 *p, u32 v)
{
#ifdef KVZ_HOSTSIM
  p[0] = (i16)(v & 0xffffu); p[1] = (i16)(v >> 16);
#else
  *(KVZ_LDS u32 *)p = v;
#endif
}
IC_DEV u32 load_mv32(const i16 *p)
{
#ifdef KVZ_HOSTSIM
  return (u32)(uint16_t)p[0] | (u32)(uint16_t)p[1] << 16;
#else
  return *(const KVZ_LDS u32 *)p;
#endif
}
// inter.c:1330-1352 kvz_inter_get_mv_cand (get_mv_cand_from_candidates :1213-1310): the two predictors as x | y << 16
IC_DEV void mv_candidates_derive(int x, int y, int w, int h, int reflist, u32 mv[2])
{
  const Cands c = cand_gather(x, y, w, h);
  const Mot &a0 = c.a0, &a1 = c.a1, &b0 = c.b0, &b1 = c.b1, &b2 = c.b2, &th = c.th, &tc = c.tc;
  int n = 0, nb_b = 0;
  u32 t = 0;
  mv[0] = mv[1] = 0;
  if (add_mvp(a0, reflist, t) || add_mvp(a1, reflist, t)) { mv[0] = t; n = 1; }  // (the scaled second pass over a0, a1 finds what the first did: one reference picture)
  const bool from_b = add_mvp(b0, reflist, t) || add_mvp(b1, reflist, t) || add_mvp(b2, reflist, t);
  if (from_b) { if (n == 0) mv[0] = t; else mv[1] = t; nb_b = 1; }
  n += nb_b;
  if (mot_valid(a0) || mot_valid(a1)) nb_b = 1; else if (n != 2) nb_b = 0;
  if (!nb_b && from_b) { if (n == 0) mv[0] = t; else mv[1] = t; n++; }
  if (n == 2 && mv[0] == mv[1]) n = 1;
  if (M->poc > 1 && n < 2 && (mot_valid(th) || mot_valid(tc))) { t = temporal_mv(mot_sel(mot_valid(th), th, tc), reflist); if (n == 0) mv[0] = t; else mv[1] = t; n++; }
  if (n < 1) mv[0] = 0;
  if (n < 2) mv[1] = 0;
}
#if KVZ_ICTU_REFS_STATE
// ... for reference index r of a P picture's list (add_mvp_candidate, inter.c:1186-1220): without scaling the neighbour must refer to the same picture -- in a P slice,
// whose one list names every picture once, the same index --, with scaling any neighbour's vector is taken and brought to the distance of entry r
IC_DEV bool add_mvp_ref(const Mot &cand, int r, bool scaling, u32 &mv)
{
  if (!mot_valid(cand) || !(cand.d & 1u)) return false;
  const int c = (int)((cand.d >> 8) & 0xffu);
  if (scaling) {
    const int scale = L->rf.spatial[r & 3][c & 3];
    if (scale != KVZ_MV_SCALE_NONE) IC_REFS_EVENT(0);
    mv = mv_scale_packed(cand.m0, scale);
    return true;
  }
  if (c != r) return false;
  mv = cand.m0;
  return true;
}
IC_DEV void mv_candidates_derive_refs(int x, int y, int w, int h, int r, u32 mv[2])  // get_mv_cand_from_candidates (inter.c:1225-1317), list 0 of a P slice
{
  const Cands c = cand_gather(x, y, w, h);
  int n = 0, nb_b = 0;
  u32 t = 0;
  mv[0] = mv[1] = 0;
  if (add_mvp_ref(c.a0, r, false, t) || add_mvp_ref(c.a1, r, false, t)) { mv[0] = t; n = 1; }
  if (n == 0 && (add_mvp_ref(c.a0, r, true, t) || add_mvp_ref(c.a1, r, true, t))) { mv[0] = t; n = 1; }
  if (add_mvp_ref(c.b0, r, false, t) || add_mvp_ref(c.b1, r, false, t) || add_mvp_ref(c.b2, r, false, t)) { if (n == 0) mv[0] = t; else mv[1] = t; nb_b = 1; }
  n += nb_b;
  if (mot_valid(c.a0) || mot_valid(c.a1)) nb_b = 1; else if (n != 2) nb_b = 0;
  if (!nb_b && (add_mvp_ref(c.b0, r, true, t) || add_mvp_ref(c.b1, r, true, t) || add_mvp_ref(c.b2, r, true, t))) { if (n == 0) mv[0] = t; else mv[1] = t; n++; }  // (no left neighbour: n <= 1 here)
  if (n == 2 && mv[0] == mv[1]) n = 1;
  if (M->poc > 1 && n < 2 && (mot_valid(c.th) || mot_valid(c.tc))) { t = temporal_mv_to(mot_sel(mot_valid(c.th), c.th, c.tc), r); if (n == 0) mv[0] = t; else mv[1] = t; n++; }
  if (n < 1) mv[0] = 0;
  if (n < 2) mv[1] = 0;
}
#endif
// into L->pu.mv_cand; ref: the reference index the predictors are for (a launch with reference lists; 0 otherwise)
IC_FN void mv_candidates(int x, int y, int w, int h, int reflist_, int ref = 0)
{
  const int reflist = reflist_ | ref << 1;  // (what the cache of the last derivation is keyed by)
  IC_COUNT(19);
  i16 (*mv_cand)[2] = L->pu.mv_cand;
  // the neighbours a PU's predictors come from are all coded before it and do not change while it is searched, priced and, later, coded
  if (L->mvc_key[0] == x && L->mvc_key[1] == y && L->mvc_key[2] == w && L->mvc_key[3] == reflist) {
    store_mv32(mv_cand[0], load_mv32(L->mvc[0])); store_mv32(mv_cand[1], load_mv32(L->mvc[1]));
    return;
  }
  u32 mv[2];
#if KVZ_ICTU_REFS_STATE
  if (KVZ_ICTU_REFS) mv_candidates_derive_refs(x, y, w, h, ref, mv); else
#endif
  mv_candidates_derive(x, y, w, h, reflist_, mv);
  L->mvc_key[0] = x; L->mvc_key[1] = y; L->mvc_key[2] = w; L->mvc_key[3] = reflist;
  store_mv32(mv_cand[0], mv[0]); store_mv32(mv_cand[1], mv[1]);
  store_mv32(L->mvc[0], mv[0]); store_mv32(L->mvc[1], mv[1]);
}
