// kvz_inter_ctu_search.inc -- part of struct InterCtu (kvz_inter_ctu.hpp): the search itself, the reference's control flow taken by every lane alike
// (oracle/kvz_oracle_inter.inc function by function).

// the keys of the first m->size entries by ascending cost, equal costs in the order they stand (the reference's insertion sort, search_inter.c kvz_sort_keys_by_cost)
IC_DEV void sort_keys(UMap *m)
{
#ifdef KVZ_HOSTSIM
  for (int i = 1; i < m->size; i++) {
    const int8_t k = m->keys[i];
    const double c = m->cost[k];
    int j = i;
    while (j > 0 && c < m->cost[m->keys[j - 1]]) { m->keys[j] = m->keys[j - 1]; j--; }
    m->keys[j] = k;
  }
#else
  // On the device in registers: the five keys and their costs in two rounds of LDS reads, the sort as adjacent exchanges on strict "less" (what the insertion does, and
  // nothing more: left of an element that stays the prefix is sorted), entries past the size at +infinity; read back cost by cost, the loop was ~20 dependent round trips
  const int n = m->size;
  if (n < 2) return;
  int k0 = m->keys[0], k1 = m->keys[1], k2 = m->keys[2], k3 = m->keys[3], k4 = m->keys[4];
  const double inf = __builtin_huge_val();
  double c0 = m->cost[k0 & 7], c1 = m->cost[k1 & 7], c2 = n > 2 ? m->cost[k2 & 7] : inf, c3 = n > 3 ? m->cost[k3 & 7] : inf, c4 = n > 4 ? m->cost[k4 & 7] : inf;
#define IC_CX(ca, ka, cb, kb) do { const bool sw_ = (cb) < (ca); const double tc_ = sw_ ? (cb) : (ca); (cb) = sw_ ? (ca) : (cb); (ca) = tc_; const int tk_ = sw_ ? (kb) : (ka); (kb) = sw_ ? (ka) : (kb); (ka) = tk_; } while (0)
  IC_CX(c0, k0, c1, k1);
  IC_CX(c1, k1, c2, k2); IC_CX(c0, k0, c1, k1);
  IC_CX(c2, k2, c3, k3); IC_CX(c1, k1, c2, k2); IC_CX(c0, k0, c1, k1);
  IC_CX(c3, k3, c4, k4); IC_CX(c2, k2, c3, k3); IC_CX(c1, k1, c2, k2); IC_CX(c0, k0, c1, k1);
#undef IC_CX
  m->keys[0] = (int8_t)k0; m->keys[1] = (int8_t)k1;
  if (n > 2) m->keys[2] = (int8_t)k2;
  if (n > 3) m->keys[3] = (int8_t)k3;
  if (n > 4) m->keys[4] = (int8_t)k4;
#endif
}
IC_DEV void set_motion(CuInfo *cu, const MCand &c)
{
  cu->mv_dir = c.dir;
  for (int l = 0; l < 2; l++) { cu->mv_ref[l] = c.ref[l]; cu->mv[l][0] = c.mv[l][0]; cu->mv[l][1] = c.mv[l][1]; }
}
// The CU record of the depth-3 CU under evaluation at (xl, yl): it lives in the decided picture's array (one record per 8x8).  The candidates of depth 1 and 2 have
// no cells of their own -- nothing reads a level's CU records inside the CU under evaluation; commit_down writes them when the CU is final.
IC_DEV void set_record(int lv, int xl, int yl)
{
  if (lv != 3) return;
  IC_FOR(tid) { if (tid == 0) *dcell(xl, yl) = L->cur_cu[3]; }
  IC_SYNC();
}

// ref: the entry of the picture's list that is searched (a launch with reference lists; 0 otherwise, the one reference picture)
IC_FN void search_pu_inter_ref(int depth, int ref = 0)
{
  PuSearch &pu = L->pu;
  UMap *amvp = L->amvp;
  IC_PROF(IP_CAND, mv_candidates(pu.x, pu.y, pu.w, pu.w, 0, ref));
  int sx = 0, sy = 0;
  const CuInfo *col_frame = ref_cu_frame();
#if KVZ_ICTU_REFS_STATE
  if (KVZ_ICTU_REFS) { use_ref(ref); col_frame = L->rf_cu[ref & (KVZ_HIP_MAX_REFS - 1)]; }  // search_inter.c:1288: the searched picture's own CU records
#endif
  const CuInfo ref_cu = load_cu(col_frame + (((K->tile_y + pu.y + (pu.w >> 1)) >> 2) * (K->ref_w >> 2) + ((K->tile_x + pu.x + (pu.w >> 1)) >> 2)));  // search_inter.c:1286-1287: the frame position
  const bool has_start = ref_cu.type == 2;
  if (has_start) { const bool l0 = (ref_cu.mv_dir & 1) != 0; sx = l0 ? ref_cu.mv[0][0] : ref_cu.mv[1][0]; sy = l0 ? ref_cu.mv[0][1] : ref_cu.mv[1][1]; }
#if KVZ_ICTU_REFS_STATE
  if (KVZ_ICTU_REFS && has_start) {  // search_inter.c:1300-1333: from the distance of the co-located CU's own reference to the distance of the searched picture
    const int scale = L->rf.start[ref & 3][((ref_cu.mv_dir & 1) ? ref_cu.mv_ref[0] : ref_cu.mv_ref[1]) & 3];
    sx = mv_scale(sx, scale); sy = mv_scale(sy, scale);
  }
#endif
  IC_PROF(IP_ME, me_integer(has_start, sx, sy));
  const decltype(InterLds::best) best = L->best;
  const bool valid = mv_allowed(best.mvx, best.mvy) && best.cost < IC_MAX_COST;
  const int mvp = select_mv_cand(best.mvx, best.mvy);
  for (int list = 0; list < IC_LISTS; list++) {  // (a P slice's L1 is empty: search_inter.c:1237-1259 finds the picture in list 0 alone)
    if (!valid) continue;
    UMap *m = &amvp[list];
    const int e = m->size;
    CuInfo *u = &m->unit[e];
    for (int i = 0; i < 11; i++) ((uint16_t *)u)[i] = ((const uint16_t *)&L->cur_cu[depth])[i];  // *u = the CU under evaluation, LDS to LDS (a record held in a local goes through the stack)
    u->type = 2; u->merged = 0; u->skipped = 0;
    u->mv_dir = (u8)(list + 1);
    u->mv[0][0] = u->mv[0][1] = u->mv[1][0] = u->mv[1][1] = 0; u->mv_ref[0] = u->mv_ref[1] = 255;
    u->mv_ref[list] = (u8)ref;
    u->mv[list][0] = (i16)best.mvx; u->mv[list][1] = (i16)best.mvy;
    u->mv_cand[0] = u->mv_cand[1] = 0;
    u->mv_cand[list] = (u8)mvp;
    m->cost[e] = best.cost; m->bits[e] = best.bits; m->keys[e] = (int8_t)e; m->size++;
  }
}

// kvz_quantize_lcu_residual of an inter CU that is one transform unit (transform.c:439-520)
// (the CU's record is L->cur_cu[depth]: its coded block flags are set here)
IC_FN void quantize_inter_cu(int lv, int x, int y, int depth, bool luma, bool chroma, bool early_skip)
{
  const int w = 64 >> depth, xl = x - cx, yl = y - cy;
  unsigned cbf = L->cur_cu[depth].cbf;
  if (luma) { cbf = cbf_clear(cbf, depth, 0); if (quantize_tu(lv, 0, xl, yl, w, false, early_skip)) cbf = cbf_set(cbf, depth, 0); }
  if (chroma) {
    cbf = cbf_clear(cbf, depth, 1); cbf = cbf_clear(cbf, depth, 2);
    for (int c = 1; c <= 2; c++) if (quantize_tu(lv, c, xl, yl, w / 2, false, early_skip)) cbf = cbf_set(cbf, depth, c);
  }
  L->cur_cu[depth].cbf = (uint16_t)cbf;
}

IC_DEV int skip_context(int x, int y)
{
  int c = 0;
  if (x) c += cell_at(x - 1, y).skipped;
  if (y) c += cell_at(x, y - 1).skipped;
  return c;
}
IC_DEV int split_model(int x, int y, int depth)
{
  int m = 0;
  if (x > 0 && cell_at(x - 1, y).depth > depth) m++;
  if (y > 0 && cell_at(x, y - 1).depth > depth) m++;
  return m;
}

// search_pu_inter (search_inter.c:1610-2055) for the 2Nx2N PU; `cur` is the CU's record, kept by every lane.  Returns true on an early skip.
IC_FN bool search_pu_inter(int lv, int x, int y, int depth)
{
  const int w = 64 >> depth, xl = x - cx, yl = y - cy;
  CuInfo &cur = L->cur_cu[depth];
  UMap *amvp = L->amvp;
  UMap &merge = L->merge;
  PuSearch &pu = L->pu;
  pu.x = x; pu.y = y; pu.w = w;
  pu.mv_cand[0][0] = pu.mv_cand[0][1] = pu.mv_cand[1][0] = pu.mv_cand[1][1] = 0;
  cur.type = 0;
  cur.depth = (u8)depth;
  cur.mv_cand[0] = cur.mv_cand[1] = 0;
  IC_PROF(IP_CAND, pu.num_merge = merge_candidates(x, y, w, w));
  const PView org0 = orgv(0, xl, yl);  // the candidates' SATDs and the motion search both compare with the PU's source block
  merge.size = 0;
  for (int i = 0; i < 5; i++) { merge.keys[i] = -1; merge.cost[i] = IC_MAX_COST; }
  const double merge_flag_cost = M->fbits[cab.s[IX_MERGE_FLAG] ^ 1];
  double best_merge_cost = IC_MAX_COST;
  for (int mi = 0; mi < pu.num_merge; mi++) {
    const MCand c = pu.merge[mi];
    set_motion(&cur, c);
    const bool dup = ((pu.merge_dup >> mi) & 1) != 0;  // (merge_candidates compared the entries while it had them in registers)
    if (((c.dir & 1) && !mv_allowed(c.mv[0][0], c.mv[0][1])) || ((c.dir & 2) && !mv_allowed(c.mv[1][0], c.mv[1][1])) || dup) continue;
    u32 merge_satd = 0;
    // the candidate's luma prediction goes into the level's samples (nothing else is there yet) and, if it is the best so far, a copy into best_luma
    const PView cand = lvl(lv, 0, xl, yl);
    IC_PROF(IP_MERGE, { inter_predict(lv, x, y, w, cur, true, false); merge_satd = satd_block(cand.p, cand.s, org0.p, org0.s, w); });
#if defined(KVZ_HOSTSIM)
    if (KVZ_ICTU_REFS && mi >= pu.zero_from && c.ref[0] > 0) IC_REFS_EVENT(2);  // a zero candidate of a reference index above 0 is evaluated
#endif
    const int e = merge.size;
    merge.unit[e] = cur;
    merge.unit[e].type = 2; merge.unit[e].merge_idx = (u8)mi; merge.unit[e].merged = 1; merge.unit[e].skipped = 0;
    const double bits = merge_flag_cost + mi + M->fbits[cab.s[IX_MERGE_IDX] ^ (mi != 0)];
    merge.cost[e] = (double)merge_satd;
    merge.cost[e] += bits * M->lambda_sqrt;
    merge.bits[e] = bits;
    merge.keys[e] = (int8_t)e;
    merge.size++;
    if (e == 0 || merge.cost[e] < best_merge_cost) {  // keep the luma prediction of what the (stable) sort will put first: the early-skip trial starts from it
      best_merge_cost = merge.cost[e];
      copy_luma(lvl(lv, 0, xl, yl), best_luma(lv), w);
    }
  }
  sort_keys(&merge);
  L->level_holds = 0;
  if (merge.size > 0) {  // early skip
    const int mi = merge.unit[merge.keys[0]].merge_idx;
    set_motion(&cur, pu.merge[mi]);
    cur.tr_depth = (u8)(depth > 1 ? depth : 1);
    IC_PROF(IP_EARLY_SKIP, {
      // kvz_inter_recon_cu of the best candidate (search_inter.c:1765): its luma prediction was kept above; a transform unit quantised with early_skip leaves the samples alone
      copy_luma(best_luma(lv), lvl(lv, 0, xl, yl), w);
      quantize_inter_cu(lv, x, y, depth, true, false, true);
    });
    L->level_holds = 1;
    if (!cbf_is_set(cur.cbf, depth, 0)) {
      IC_PROF(IP_EARLY_SKIP, { inter_predict(lv, x, y, w, cur, false, true); quantize_inter_cu(lv, x, y, depth, false, true, true); });
      L->level_holds = 3;
      if (!cbf_any(cur.cbf, depth)) {
        cur.type = 2; cur.merge_idx = (u8)mi; cur.skipped = 1;
        merge.size = 1;
        merge.cost[0] = 0.0;
        merge.bits[0] = mi;
        merge.unit[0] = cur;
        return true;
      }
    }
  }
  if (KVZ_ICTU_P) amvp[0].size = 0;
  else amvp[0].size = amvp[1].size = 0;  // (kvazaar's third list, the bi-prediction search of search_inter.c:1919-2034, needs two reference pictures)
  for (int d = 0; d < IC_LISTS; d++) { amvp[d].cost[0] = IC_MAX_COST; amvp[d].keys[0] = 0; }
#if KVZ_ICTU_REFS_STATE
  if (KVZ_ICTU_REFS) { for (int r = 0; r < list_length(); r++) search_pu_inter_ref(depth, r); } else  // search_inter.c:1807-1812: every picture of the list
#endif
  search_pu_inter_ref(depth);
  sort_keys(&amvp[0]);
  if (!KVZ_ICTU_P) sort_keys(&amvp[1]);
  int best_keys[2] = { amvp[0].size > 0 ? amvp[0].keys[0] : 0, !KVZ_ICTU_P && amvp[1].size > 0 ? amvp[1].keys[0] : 0 };
  if (!KVZ_ICTU_P && amvp[0].size > 0 && amvp[1].size > 0) {  // (search_inter.c:1831 cfg->bipred: a P slice has one list, nothing to eliminate)
    const double l0_2nd = amvp[0].size > 1 ? amvp[0].cost[amvp[0].keys[1]] : IC_MAX_COST, l1_2nd = amvp[1].size > 1 ? amvp[1].cost[amvp[1].keys[1]] : IC_MAX_COST;
    const int list = l0_2nd <= l1_2nd ? 1 : 0;
    amvp[list].cost[best_keys[list]] = IC_MAX_COST;
    sort_keys(&amvp[list]);
    amvp[list].size--;
    best_keys[list] = amvp[list].keys[0];
  }
  for (int list = 0; list < IC_LISTS; list++) {
    const int n_best = amvp[list].size < 1 ? amvp[list].size : 1;
    if (M->fme_level > 0) {
      for (int i = 0; i < n_best; i++) {
        const int key = amvp[list].keys[i];
        CuInfo *u = &amvp[list].unit[key];
#if KVZ_ICTU_REFS_STATE
        if (KVZ_ICTU_REFS) { use_ref(u->mv_ref[list]); mv_candidates(x, y, w, w, list, u->mv_ref[list]); } else  // search_inter.c:1871-1883: the picture and the predictors of the entry's reference index
#endif
        mv_candidates(x, y, w, w, list);
        L->frac.mv[0] = u->mv[list][0]; L->frac.mv[1] = u->mv[list][1];
        bool frac_ok = false;
        IC_PROF(IP_FME, frac_ok = me_fractional());
        if (!frac_ok) continue;
        const int frac_mv[2] = { L->frac.mv[0], L->frac.mv[1] };
        double frac_cost = L->frac.cost, frac_bits = L->frac.bits;
        const int mvp = select_mv_cand(frac_mv[0], frac_mv[1]);
        int extra_bits = list;
#if KVZ_ICTU_REFS_STATE
        if (KVZ_ICTU_REFS) extra_bits += u->mv_ref[list];  // search_inter.c:1897-1899 mv_ref_coded
#endif
        frac_cost += extra_bits * M->lambda_sqrt;
        frac_bits += extra_bits;
        if (mv_allowed(frac_mv[0], frac_mv[1])) {
          u->mv[list][0] = (i16)frac_mv[0]; u->mv[list][1] = (i16)frac_mv[1];
          u->mv_cand[list] = (u8)mvp;
          amvp[list].cost[key] = frac_cost;
          amvp[list].bits[key] = frac_bits;
        }
      }
      for (int i = n_best; i < amvp[list].size; i++) amvp[list].cost[amvp[list].keys[i]] = IC_MAX_COST;
    }
    sort_keys(&amvp[list]);
    amvp[list].size = n_best;
  }
  {
    const int sk = skip_context(x, y);
    const double no_skip_flag = M->fbits[cab.s[IX_SKIP + sk] ^ 0], pred_mode_bits = M->fbits[cab.s[IX_PRED_MODE] ^ 0];
    const double total_bits = no_skip_flag + 0 + pred_mode_bits;
    for (int i = 0; i < IC_LISTS; i++) if (amvp[i].size > 0) {
      const int k = amvp[i].keys[0];
      amvp[i].bits[k] += total_bits;
      amvp[i].cost[k] += total_bits * M->lambda_sqrt;
    }
  }
  return false;
}

// results: L->inter_cost, L->inter_bitcost, the CU's record L->cur_cu[depth]
IC_FN_INTER void search_cu_inter(int lv, int x, int y, int depth)
{
  UMap *amvp = L->amvp;
  UMap &merge = L->merge;
  CuInfo &cur = L->cur_cu[depth];
  double *inter_cost = &L->inter_cost, *inter_bitcost = &L->inter_bitcost;
  *inter_cost = IC_MAX_COST;
  *inter_bitcost = IC_MAX_INT;
  if (search_pu_inter(lv, x, y, depth)) { *inter_cost = merge.cost[0]; *inter_bitcost = merge.bits[0]; return; }
  int which = -1, wk = 0;
  for (int d = 0; d < IC_LISTS; d++) {
    const int k = amvp[d].keys[0];
    if (amvp[d].size > 0 && amvp[d].cost[k] < *inter_cost) { which = d; wk = k; *inter_cost = amvp[d].cost[k]; *inter_bitcost = amvp[d].bits[k]; }
  }
  if (merge.size > 0 && merge.cost[merge.keys[0]] < *inter_cost) { which = 3; wk = merge.keys[0]; *inter_cost = merge.cost[wk]; *inter_bitcost = 0; }
  if (*inter_cost == IC_MAX_COST) { *inter_bitcost = IC_MAX_INT; return; }
  cur = which == 3 ? merge.unit[wk] : amvp[which].unit[wk];
  // kvz_inter_recon_cu of the winner (search_inter.c:2270-2280); when that is the best merge candidate the trial above has left (part of) its prediction in the level
  const int have = (which == 3 && wk == merge.keys[0]) ? L->level_holds : 0;
  IC_PROF(IP_WINNER_MC, inter_predict(lv, x, y, 64 >> depth, cur, !(have & 1), !(have & 2)));
}

// ---- bits ----
IC_DEV unsigned ep_ex_golomb_bins(unsigned symbol, unsigned count)
{
  unsigned n = 0;
  while (symbol >= (1u << count)) { n++; symbol -= 1u << count; count++; }
  return n + 1 + count;
}
IC_DEV double mvd_syntax_bits(int hor, int ver, bool update)
{
  double bits = 0;
  const unsigned ah = (unsigned)iabs(hor), av = (unsigned)iabs(ver);
  bits += price(IX_MVD, hor != 0, update);
  bits += price(IX_MVD, ver != 0, update);
  if (hor) bits += price(IX_MVD + 1, ah > 1, update);
  if (ver) bits += price(IX_MVD + 1, av > 1, update);
  if (hor) { if (ah > 1) bits += ep_ex_golomb_bins(ah - 2, 1); bits += 1; }
  if (ver) { if (av > 1) bits += ep_ex_golomb_bins(av - 2, 1); bits += 1; }
  return bits;
}
IC_DEV double merge_idx_bits(int merge_idx, bool update)
{
  double bits = 0;
  for (int ui = 0; ui < 4; ui++) {
    const int symbol = ui != merge_idx;
    if (ui == 0) bits += price(IX_MERGE_IDX, symbol, update); else bits += 1;
    if (!symbol) break;
  }
  return bits;
}
#if KVZ_ICTU_REFS_STATE
// ref_idx_lX of a list of n > 1 entries (encode_coding_tree.c:359-383): truncated unary, two context-coded bins, bypass from the third on
IC_DEV double ref_idx_bits(int ref, int n, bool update)
{
  double bits = price(IX_REF_IDX, ref != 0, update);
  if (ref > 0)
    for (int i = 0; i < n - 2; i++) {
      const int symbol = i == ref - 1 ? 0 : 1;
      if (i == 0) bits += price(IX_REF_IDX + 1, symbol, update); else bits += 1;
      if (!symbol) break;
    }
  return bits;
}
#endif
IC_FN double inter_pu_bits(int x, int y, int depth, const CuInfo cu, bool update)
{
  const int w = 64 >> depth;
  double bits = price(IX_MERGE_FLAG, cu.merged, update);
  if (cu.merged) return bits + merge_idx_bits(cu.merge_idx, update);
  if (!KVZ_ICTU_P) {  // inter_pred_idc is B-slice syntax (encode_coding_tree.c:339)
    const int inter_dir = cu.mv_dir - 1;
    bits += price(IX_INTER_DIR + depth, inter_dir == 2, update);
    if (inter_dir < 2) bits += price(IX_INTER_DIR + 4, inter_dir, update);
  }
  for (int l = 0; l < IC_LISTS; l++) {
    if (!(cu.mv_dir & (1 << l))) continue;
#if KVZ_ICTU_REFS_STATE
    if (KVZ_ICTU_REFS) {
      if (list_length() > 1) bits += ref_idx_bits(cu.mv_ref[l], list_length(), update);
      mv_candidates(x, y, w, w, l, cu.mv_ref[l]);
    } else
#endif
    mv_candidates(x, y, w, w, l);
    const int k = cu.mv_cand[l];
    bits += mvd_syntax_bits(cu.mv[l][0] - L->pu.mv_cand[k][0], cu.mv[l][1] - L->pu.mv_cand[k][1], update);
    bits += price(IX_MVP_IDX, k, update);
  }
  return bits;
}
IC_DEV void mpm_candidates(int y, bool has_left, const CuInfo &left, bool has_above, const CuInfo &above, int8_t preds[3])
{
  int l = 1, a = 1;
  if (has_left && left.type == 1) l = left.mode;
  if (has_above && above.type == 1 && y % 64 != 0) a = above.mode;
  intra_mpm(l, a, preds);
}
IC_DEV double luma_mode_bits(int mode, const int8_t preds[3], bool update)
{
  double bits = 0;
  int in = 0;
  for (int i = 0; i < 3; i++) if (mode == preds[i]) in = 1;
  bits += price(IX_INTRA, in, update);
  if (in) bits += (mode == preds[0]) ? 1 : 2; else bits += 5;
  return bits;
}
IC_FN double intra_mode_syntax_bits(int x, int y, int mode, bool update, bool mock)
{
  CuInfo lc = zero_cu(), ac = zero_cu();
  bool hl = false, ha = false;
  if (x > 0 && !(mock && x % 64 == 0)) { lc = cell_at(x - 1, y); hl = true; }
  if (y % 64 > 0 && y > 0) { ac = cell_at(x, y - 1); ha = true; }
  int8_t preds[3];
  mpm_candidates(y, hl, lc, ha, ac, preds);
  double bits = luma_mode_bits(mode, preds, update);
  bits += price(IX_CHROMA, 0, update);
  return bits;
}
IC_FN double mock_encode_b(int x, int y, int depth, const CuInfo cu, bool update)
{
  double bits = 0;
  const int w = 64 >> depth;
  if (depth != 3 && !(F.W < x + w || F.H < y + w)) bits += price(IX_SPLIT + split_model(x, y, depth), 0, update);
  bits += price(IX_SKIP + skip_context(x, y), cu.skipped, update);
  if (cu.skipped) return bits + merge_idx_bits(cu.merge_idx, update);
  bits += price(IX_PRED_MODE, cu.type == 1, update);
  if (cu.type == 2 || depth == 3) bits += price(IX_PART, 1, update);
  if (cu.type == 2) bits += inter_pu_bits(x, y, depth, cu, update);
  else bits += intra_mode_syntax_bits(x, y, cu.mode, update, true);
  return bits;
}

// cu_rd_cost_tr_split_accurate (search.c:425-550) of a CU whose transform tree is one unit (depth >= 1); coefficients priced as kvz_get_coeff_cost does (rdo.c:311-340):
// the fast estimate the quantisation left in ccost, or -- picture QP >= 28 -- the residual coder in counting mode on the search contexts, luma then Cb then Cr, after
// the tree's own flags as the reference orders them
IC_FN double rd_cost_b(int lv, int xl, int yl, int depth, const CuInfo pred, bool update)
{
  const int width = 64 >> depth;
  const bool skip_residual = pred.skipped || (pred.type == 2 && pred.cbf == 0);
  double coeff_bits = 0, tr_tree_bits = 0;
  const bool cb_y = cbf_is_set(pred.cbf, depth, 0), cb_u = cbf_is_set(pred.cbf, depth, 1), cb_v = cbf_is_set(pred.cbf, depth, 2);
  if (pred.type == 2 && !pred.merged) tr_tree_bits += price(IX_ROOT_CBF, cbf_any(pred.cbf, depth), update);
  if (!skip_residual) {
    tr_tree_bits += price(IX_CBF_CHROMA, cb_u, update);
    tr_tree_bits += price(IX_CBF_CHROMA, cb_v, update);
    if (pred.type == 1 || cb_u || cb_v) tr_tree_bits += price(IX_CBF_LUMA + 1, cb_y, update);
  }
  const int cw = depth <= 3 ? 64 >> (depth + 1) : 64 >> depth;
  ssd_cu(lv, xl, yl, width, cw);
  const u32 luma_ssd = L->ssd[0], chroma_ssd = L->ssd[1];
  if (!skip_residual) {
    if (M->coeff_cabac) {
      const int scan = pred.type == 1 ? intra_scan_order(pred.mode, depth) : 0;
      if (cb_y) coeff_bits += coeff_bits_cabac(coef(lv, 0, xl, yl), ilog2i(width), 0, scan, update);
      if (cb_u) coeff_bits += coeff_bits_cabac(coef(lv, 1, xl, yl), ilog2i(cw), 2, scan, update);
      if (cb_v) coeff_bits += coeff_bits_cabac(coef(lv, 2, xl, yl), ilog2i(cw), 2, scan, update);
    } else {
      if (cb_y) coeff_bits += L->ccost[0];
      if (cb_u) coeff_bits += L->ccost[1];
      if (cb_v) coeff_bits += L->ccost[2];
    }
  }
  const double bits = tr_tree_bits + coeff_bits;
  return luma_ssd * 0.8 + chroma_ssd * 1.5 + bits * M->lambda;
}

// ---- the intra alternative (oracle search_cu_intra_cost / rough_search, recon_cu) ----
// returns the mode, its cost in L->intra_cost
IC_FN_INTRA int search_cu_intra(int x, int y, int depth)
{
  const int log2w = 6 - depth, xl = x - cx, yl = y - cy;
  CuInfo lc = zero_cu(), ac = zero_cu();
  bool hl = false, ha = false;
  if (x >= 4) { lc = cell_at(x - 1, y); hl = true; }
  if (y >= 4 && yl > 0) { ac = cell_at(x, y - 1); ha = true; }
  int8_t preds[3], *modes = L->modes;
  double *costs = L->costs;
  mpm_candidates(y, hl, lc, ha, ac, preds);
  build_reference(log2w, 0, x, y);
  int n = 0, offset = log2w == 2 ? 2 : (log2w == 3 ? 4 : 8);  // search_intra.c:433 { 2, 4, 8, 8 }[log2w - 2]
  L->intra_done = 0;
  unsigned long long want = (1ull << preds[0]) | (1ull << preds[1]) | (1ull << preds[2]) | 3ull;  // the modes added at the end are known from the start
  for (int mode = 2; mode <= 34; mode += offset) want |= 1ull << mode;
  (void)want;
  intra_all_mode_costs(log2w, xl, yl);  // every mode's cost at once; the reference's selection is then replayed on the table (the later requests find it complete)
  i32 min_cost = 0x7fffffff, max_cost = -0x7fffffff - 1;
  for (int mode = 2; mode <= 34; mode += 2 * offset)
    for (int i = 0; i < 2; i++) if (mode + i * offset <= 34) {
      costs[n] = (double)L->mcost[mode + i * offset]; modes[n] = (int8_t)(mode + i * offset);
      if (costs[n] < min_cost) min_cost = (i32)costs[n];
      if (costs[n] > max_cost) max_cost = (i32)costs[n];
      n++;
    }
  int bi = 0;
  for (int i = 1; i < n; i++) if (costs[i] < costs[bi]) bi = i;
  int8_t best_mode = modes[bi];
  double best_cost = min_cost;
  if (min_cost != max_cost) {
    while (offset > 1) {
      offset >>= 1;
      const int8_t tm[2] = { (int8_t)(best_mode - offset), (int8_t)(best_mode + offset) };
      want = 0;
      for (int i = 0; i < 2; i++) if (tm[i] >= 2 && tm[i] <= 34) want |= 1ull << tm[i];
      intra_mode_costs(log2w, xl, yl, want);
      for (int i = 0; i < 2; i++) if (tm[i] >= 2 && tm[i] <= 34) {
        costs[n] = (double)L->mcost[tm[i]]; modes[n] = tm[i];
        n++;
      }
      // both probes of a step are compared with the best BEFORE the step in the reference's order: first, then second
      const int first = n - ((tm[0] >= 2 && tm[0] <= 34) + (tm[1] >= 2 && tm[1] <= 34));
      for (int i = first; i < n; i++) if (costs[i] < best_cost) { best_cost = costs[i]; best_mode = modes[i]; }
    }
  }
  const int8_t add_modes[5] = { preds[0], preds[1], preds[2], 0, 1 };
  for (int p = 0; p < 5; p++) {
    bool has = false;
    for (int i = 0; i < n; i++) if (modes[i] == add_modes[p]) { has = true; break; }
    if (!has) { costs[n] = (double)L->mcost[add_modes[p]]; modes[n] = add_modes[p]; n++; }
  }
  for (int i = 0; i < n; i++) costs[i] += M->lambda_sqrt * luma_mode_bits(modes[i], preds, false);
  bi = 0;
  for (int i = 1; i < n; i++) if (costs[i] < costs[bi]) bi = i;
  L->intra_cost = costs[bi];
  return modes[bi];
}
// kvz_intra_recon_cu (intra.c:623-717) for a CU of depth 2 or 3: predict + transform unit per plane; sets the coded block flags of `cu`
// (the CU's record is L->cur_cu[depth])
IC_FN_INTRA void recon_cu_intra(int lv, int x, int y, int depth, bool luma, bool chroma)
{
  const int xl = x - cx, yl = y - cy, log2w = 6 - depth, mode = L->cur_cu[depth].mode;
  unsigned cbf = L->cur_cu[depth].cbf;
  for (int c = 0; c < 3; c++) {
    if ((c == 0 && !luma) || (c > 0 && !chroma)) continue;
    const int l2 = c ? (depth >= 3 ? 2 : log2w - 1) : log2w, w = 1 << l2;
    cbf = cbf_clear(cbf, depth, c);
    build_reference(l2, c, x, y);
    const PView rv = lvl(lv, c, xl, yl);
    IC_FOR(tid) { for (int i = tid; i < w * w; i += KVZ_ICTU_THREADS) rv.p[(i >> l2) * rv.s + (i & (w - 1))] = intra_pixel(l2, mode, c, i & (w - 1), i >> l2); }
    IC_SYNC();
    if (quantize_tu(lv, c, xl, yl, w, true, false)) cbf = cbf_set(cbf, depth, c);
  }
  L->cur_cu[depth].cbf = (uint16_t)cbf;
}

// ---- search_cu of a B slice (search.c:646-1063), one instantiation per depth ----
// the position of the depth-d CU whose subtree is being searched: the child indices of the depths above it
IC_DEV int depth_x(int d) { int v = cx; for (int k = 0; k < d; k++) v += (L->child[k] & 1) * (32 >> k); return v; }
IC_DEV int depth_y(int d) { int v = cy; for (int k = 0; k < d; k++) v += (L->child[k] >> 1) * (32 >> k); return v; }
#ifndef KVZ_ICTU_INLINE_FROM
#define KVZ_ICTU_INLINE_FROM 4  /* every depth a call (85 per CTU): with depth 3 inside its parent's body (21 calls) the bigger functions spill in their hot paths -- 341 k
                                   CTUs/s against 373 k, 306 k with depth 2 inlined as well (profiles/experiments/README.md, r04_v) */
#endif
template <int DEPTH> IC_FN double search_cu_body(int x, int y)
{
  constexpr int depth = DEPTH, lv = DEPTH, w = 64 >> DEPTH;
  const int xl = x - cx, yl = y - cy;
  double cost = IC_MAX_COST, inter_zero_coeff_cost = IC_MAX_COST, inter_bitcost = IC_MAX_INT;
  ICtxL &pre_search = L->pre[DEPTH];
  IC_PROF(IP_CTX, ctx_copy_words(IC_CTX_L(pre_search), IC_CTX_L(cab)));
  if (x >= F.W || y >= F.H) return 0;
  CuInfo &cur = L->cur_cu[DEPTH];
  cur = zero_cu();  // the level's cells of a region are still as init_lcu_t left them when its CU is first (and only once) evaluated there
  if (DEPTH == 1) IC_PROF(IP_IO, load_org_quadrant(x, y));
  cur.depth = (u8)(depth > 3 ? 3 : depth);
  cur.tr_depth = (u8)(depth > 0 ? depth : 1);
  cur.type = 0;
  const bool inside = x + w <= F.W && y + w <= F.H;
  if (inside) {
    // search.c:702-713: pu_depth_inter.min .. max -- or, whatever the depth, a CU inside a block of the smallest inter size that the picture edge cuts (the split down to
    // it was forced: `ultrafast` / `superfast` with a width or height that is 8 mod 16)
    const int wmin = 64 >> M->pu_depth_inter_max;
    if ((depth >= 1 && depth <= M->pu_depth_inter_max) || (x & ~(wmin - 1)) + wmin > F.W || (y & ~(wmin - 1)) + wmin > F.H) {
      search_cu_inter(lv, x, y, depth);
      const double mode_cost = L->inter_cost, mode_bitcost = L->inter_bitcost;
      if (mode_cost < cost) { cost = mode_cost; inter_bitcost = mode_bitcost; cur.type = 2; }
    }
    const bool skip_intra = (cur.type != 0 && cost / (w * w) < 8) || cur.skipped;
    if (depth >= 2 && depth <= 3 && !skip_intra) {
      int mode = 0;
      IC_PROF(IP_INTRA_SEARCH, mode = search_cu_intra(x, y, depth));
      const double intra_cost = L->intra_cost;
      if (intra_cost < cost) { cost = intra_cost; cur.type = 1; cur.mode = (u8)mode; cur.skipped = 0; cur.merged = 0; cur.tr_depth = (u8)depth; }
    }
    if (cur.type == 1) {
      IC_PROF(IP_INTRA_RECON, { recon_cu_intra(lv, x, y, depth, true, false); recon_cu_intra(lv, x, y, depth, false, true); });
    } else if (cur.type == 2) {
      if (!cur.skipped) {
        cur.tr_depth = (u8)(depth > 1 ? depth : 1);
        // search.c:833 predicts the CU again here (kvz_inter_recon_cu); kvz_search_cu_inter has just left exactly that prediction in this level, and nothing wrote it since
        IC_PROF(IP_ZERO_COEFF, {
          double ssd = 0.0;
          ssd_cu(lv, xl, yl, w, w / 2);
          ssd += 0.8 * L->ssd[0];
          ssd += 1.5 * L->ssd[1];
          // cu_zero_coeff_cost's copy of the prediction into the next level's pixels (search.c:222)
          copy_cu_samples(lv, xl, yl, w, true);
          inter_zero_coeff_cost = ssd + inter_bitcost * M->lambda;
        });
        IC_PROF(IP_INTER_RECON, quantize_inter_cu(lv, x, y, depth, true, true, false));
        if (cur.merged && !cbf_any(cur.cbf, depth)) { cur.merged = 0; cur.skipped = 1; }
      }
      cur.type = 2;
    }
  }
  if (cur.type == 1 || cur.type == 2) {
    set_record(lv, xl, yl);
    double bits = 0;
    IC_PROF(IP_COST, { bits = mock_encode_b(x, y, depth, cur, true); cost = bits * M->lambda; cost += rd_cost_b(lv, xl, yl, depth, cur, true); });
    if (inter_zero_coeff_cost <= cost) {
      cost = inter_zero_coeff_cost;
      copy_cu_samples(lv, xl, yl, w, false);
      if (cur.merged) { cur.merged = 0; cur.skipped = 1; }
      cur.cbf = 0;
      set_record(lv, xl, yl);
    }
  }
  const bool can_split = cur.type == 0 || depth < 3;
  if (can_split) {
    if constexpr (DEPTH < 3) {
      const int half = w / 2;
      double split_cost = 0.0;
      const bool cbf = cbf_any(cur.cbf, depth);
      ICtxL &post_search = L->post[DEPTH];
      IC_PROF(IP_CTX, { ctx_copy_words(IC_CTX_L(post_search), IC_CTX_L(cab)); ctx_copy_words(IC_CTX_L(cab), IC_CTX_L(pre_search)); });
      double split_bits = 0;
      split_bits += price(IX_SPLIT + split_model(x, y, depth), 1, true);
      split_cost += split_bits * M->lambda;
      if (cur.type == 0 || cbf) {
        // what this depth needs after its children waits in LDS, so that a child's body starts with empty registers.  The children of a depth below
        // KVZ_ICTU_INLINE_FROM are inlined into it (one site: the loop), the others are calls -- a callee of this size saves ~60 registers in its prologue
        L->fr[DEPTH].cost = cost; L->fr[DEPTH].split_cost = split_cost;
        IC_SYNC();
        for (L->child[DEPTH] = 0; L->child[DEPTH] < 4; L->child[DEPTH]++) {
          if (!(L->fr[DEPTH].split_cost < L->fr[DEPTH].cost)) continue;
          const int child = L->child[DEPTH];
          double c;
          if constexpr (DEPTH + 1 >= KVZ_ICTU_INLINE_FROM) c = search_cu_body<DEPTH + 1>(depth_x(DEPTH) + (child & 1) * half, depth_y(DEPTH) + (child >> 1) * half);
          else c = search_cu_b<DEPTH + 1>(depth_x(DEPTH) + (child & 1) * half, depth_y(DEPTH) + (child >> 1) * half);
          L->fr[DEPTH].split_cost += c;
          IC_SYNC();
        }
        cost = L->fr[DEPTH].cost; split_cost = L->fr[DEPTH].split_cost;
      } else {
        split_cost = 2147483647;
      }
      // combine_intra_cus (search.c:996-1044) needs an unset CU whose first child is an intra CU of depth + 1: in a P / B slice a CU inside the picture is never
      // unset where inter prediction may be used (depth 1-3: the zero merge candidate always exists), and at depth 0 the child at depth 1 is never intra
      if (split_cost < cost) {
        cost = split_cost;  // the children's results already are the decided picture (copying level lv + 1 up is nothing here)
      } else if (depth > 0) {
        IC_PROF(IP_CTX, ctx_copy_words(IC_CTX_L(cab), IC_CTX_L(post_search)));
        IC_PROF(IP_COPY, commit_down(depth, depth_x(DEPTH) - cx, depth_y(DEPTH) - cy));
      }
    }
  } else if (depth < 4) {
    IC_PROF(IP_COPY, commit_down(depth, xl, yl));
  }
  return cost;
}
template <int DEPTH> IC_FN_CALL double search_cu_b(int x, int y) { return search_cu_body<DEPTH>(x, y); }  // ... as a call

// ---- the finished CTU's syntax on the row coder's contexts (oracle code_coding_tree_b) ----
// encode_transform_unit (encode_coding_tree.c:117-190) of a CU that is one transform unit: the residual moves its own contexts, which the next CTU's prices start from
IC_FN void code_residual(int xl, int yl, int depth, int scan, bool cb_y, bool cb_u, bool cb_v)
{
  const int w = 64 >> depth, cw = depth == 3 ? 4 : w / 2;
  if (cb_y) coeff_bits_cabac(coef(3, 0, xl, yl), ilog2i(w), 0, scan, true);
  if (cb_u) coeff_bits_cabac(coef(3, 1, xl, yl), ilog2i(cw), 2, scan, true);
  if (cb_v) coeff_bits_cabac(coef(3, 2, xl, yl), ilog2i(cw), 2, scan, true);
}
template <int DEPTH> IC_FN_CALL void code_coding_tree_b(int x, int y)
{
  constexpr int depth = DEPTH;
  const int w = 64 >> depth, half = w / 2;
  const CuInfo cur = load_dcell(x - cx, y - cy);
  const bool split_flag = cur.depth > depth;
  const bool border_x = F.W < x + w, border_y = F.H < y + w, border = border_x || border_y;
  const bool border_split_x = F.W >= x + 8 + half, border_split_y = F.H >= y + 8 + half;
  if constexpr (DEPTH != 3) {
    if (!border) price(IX_SPLIT + split_model(x, y, depth), split_flag, true);
    if (split_flag || border) {
      for (int child = 0; child < 4; child++) {
        const bool coded = child == 0 || (child == 1 && (!border_x || border_split_x)) || (child == 2 && (!border_y || border_split_y)) || (child == 3 && (!border || (border_split_x && border_split_y)));
        if (coded) code_coding_tree_b<DEPTH + 1>(x + (child & 1) * half, y + (child >> 1) * half);
      }
      return;
    }
  }
  price(IX_SKIP + skip_context(x, y), cur.skipped, true);
  if (cur.skipped) { merge_idx_bits(cur.merge_idx, true); return; }
  price(IX_PRED_MODE, cur.type == 1, true);
  if (cur.type == 2 || depth == 3) price(IX_PART, 1, true);
  const bool cb_y = cbf_is_set(cur.cbf, depth, 0), cb_u = cbf_is_set(cur.cbf, depth, 1), cb_v = cbf_is_set(cur.cbf, depth, 2);
  if (cur.type == 2) {
    inter_pu_bits(x, y, depth, cur, true);
    const bool cbf = cbf_any(cur.cbf, depth);
    if (!cur.merged) price(IX_ROOT_CBF, cbf, true);
    if (cbf) {
      price(IX_CBF_CHROMA, cb_u, true);
      price(IX_CBF_CHROMA, cb_v, true);
      if (cb_u || cb_v) price(IX_CBF_LUMA + 1, cb_y, true);
      if (M->coeff_cabac) code_residual(x - cx, y - cy, depth, 0, cb_y, cb_u, cb_v);
    }
  } else {
    intra_mode_syntax_bits(x, y, cur.mode, true, false);
    price(IX_CBF_CHROMA, cb_u, true);
    price(IX_CBF_CHROMA, cb_v, true);
    price(IX_CBF_LUMA + 1, cb_y, true);
    if (M->coeff_cabac) code_residual(x - cx, y - cy, depth, intra_scan_order(cur.mode, depth), cb_y, cb_u, cb_v);
  }
}

// ---- one CTU ----
IC_FN void run()
{
  const int ctus = F.wc * F.hc, ix = cx >> 6, iy = cy >> 6;
  // the row coder's contexts at the start of this CTU (oracle kvz_oracle_lowdelay_encode's row handling; encoderstate.c:763-771)
  const ICtx *co = F.ctx_out + (long)frame * ctus, *from = nullptr;
  if (ix > 0) from = &co[iy * F.wc + ix - 1];
  else if (iy == 0) from = nullptr;
  else if (M->no_wpp) from = &co[(iy - 1) * F.wc + F.wc - 1];
  else if (F.wc > 1) from = &co[(iy - 1) * F.wc + 1];
  if (from) ctx_copy_words(IC_CTX_L(cab), IC_CTX_G(from)); else ctx_copy_words(IC_CTX_L(cab), (const KVZ_GLB u32 *)g_ic.model->ctx_init);
  ctx_copy_words(IC_CTX_L(L->row), IC_CTX_L(cab));
  L->mvc_key[2] = 0;
  IC_PROF(IP_IO, clear_cu_records());
  IC_PROF(IP_TOTAL, search_cu_b<0>(cx, cy));
  // copy_lcu_to_cu_data (search.c:1183-1207): the CU records (every 4x4 unit of an 8x8 gets the 8x8's record); the samples and the levels are in place already
  const int xmax = cx + 64 < F.W ? 64 : F.W - cx, ymax = cy + 64 < F.H ? 64 : F.H - cy;
  IC_FOR(tid) {
    for (int i = tid; i < 256; i += KVZ_ICTU_THREADS) {
      const int yy = (i >> 4) * 4, xx = (i & 15) * 4;
      if (xx < xmax && yy < ymax) store_cu((CuInfo *)g_ic.cu_frame + (((cy + yy) >> 2) * (F.W >> 2) + ((cx + xx) >> 2)), load_dcell(xx, yy));
    }
  }
  IC_SYNC();
  ctx_copy_words(IC_CTX_L(cab), IC_CTX_L(L->row));
  IC_PROF(IP_SYNTAX, code_coding_tree_b<0>(cx, cy));
  ctx_copy_words(IC_CTX_G(&F.ctx_out[(long)frame * ctus + iy * F.wc + ix]), IC_CTX_L(cab));
}
