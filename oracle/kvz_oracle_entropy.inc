/* kvz_oracle_entropy.inc -- part of kvz_oracle_ctu.c (TEST INFRASTRUCTURE, like the rest of oracle/): the entropy coder in its REAL mode.
 *
 * What kvazaar writes as slice data for an I picture, restated: the arithmetic coder (cabac.c:85-270: kvz_cabac_start, kvz_cabac_encode_bin, _bin_ep, _bins_ep,
 * _bin_trm, kvz_cabac_write, kvz_cabac_finish), the per-LCU syntax of encoder_state_worker_encode_lcu_bitstream (encoderstate.c:676-745: SAO syntax :467-552,
 * kvz_encode_coding_tree, end_of_slice_segment_flag, end_of_subset_one_bit, the substream's flush and byte alignment), the coding tree of an I slice
 * (encode_coding_tree.c:745-900 kvz_encode_coding_tree, :467-652 encode_intra_coding_unit, :193-310 encode_transform_coeff, :117-190 encode_transform_unit,
 * :63-115 kvz_encode_last_significant_xy) and the residual coder (strategies/generic/encode_coding_tree-generic.c:40-283 kvz_encode_coeff_nxn_generic with
 * cabac.c:275-301 kvz_cabac_write_coeff_remain), with the WPP context hand-over of encoderstate.c:763-771.
 *
 * The syntax writer produces a sequence of BINS through three calls -- a context-coded bin, a run of bypass bins, a terminating bin -- and the arithmetic coder
 * consumes them; the device splits the work at the same seam (kvz_entropy.hpp: bin lists per CTU, then one coder per substream).
 *
 * The bytes are those of kvazaar's per-row bitstream_t objects, i.e. WITH the emulation prevention bytes kvz_bitstream_put_byte inserts as it writes (bitstream.c:212-223);
 * their sizes are what the slice header codes as entry points.
 *
 * Pinned against the reference encoder: tests/test_entropy_oracle.py takes bitstreams kvazaar_ref wrote (committed fixtures and, where oracle/_ref exists, live runs)
 * and checks that the payload of every slice NAL ENDS with these substreams and that the entry points coded in its slice header are these substreams' sizes. */

typedef struct { uint8_t *buf; size_t cap, n; uint32_t acc; int acc_bits; int overflow; int zerocount; } ebits_t;  /* bitstream.c: put_byte / put / align_zero */
static void eb_write(ebits_t *b, uint32_t byte)
{
  if (b->n < b->cap) b->buf[b->n] = (uint8_t)byte; else b->overflow = 1;
  b->n++;
}
static void eb_put_byte(ebits_t *b, uint32_t byte)  /* bitstream.c:212-223 kvz_bitstream_put_byte: the emulation prevention byte goes in as the stream is written */
{
  byte &= 0xff;
  if (b->zerocount == 2 && byte < 4) { eb_write(b, 3); b->zerocount = 0; }
  b->zerocount = byte == 0 ? b->zerocount + 1 : 0;
  eb_write(b, byte);
}
static void eb_put(ebits_t *b, uint32_t data, int bits)
{
  while (bits-- > 0) {
    b->acc = (b->acc << 1) | ((data >> bits) & 1);
    if (++b->acc_bits == 8) { eb_put_byte(b, b->acc & 0xff); b->acc = 0; b->acc_bits = 0; }
  }
}
static void eb_align_zero(ebits_t *b) { if (b->acc_bits) eb_put(b, 0, 8 - b->acc_bits); }

typedef struct {
  uint32_t low, range, buffered_byte;
  int bits_left, num_buffered_bytes;
  uint8_t ctx[CX_ALL + 4];  /* uc_state of every context these configurations code with: KVZ_HIP_CX_* order, then the B-slice contexts CXB_* (kvz_oracle_ctu.c) */
  ebits_t *out;
  uint32_t *rec; int rec_n, rec_cap;     /* rec != NULL: the bins are listed as records (include/kvz_hip.h kvz_hip_coeff_nxn_bins) instead of being coded */
} ecabac_t;

static const uint8_t e_lps_table[64][4] = {  /* cabac.c:66-82 kvz_g_auc_lpst_table (H.265 table 9-46) */
  {128, 176, 208, 240}, {128, 167, 197, 227}, {128, 158, 187, 216}, {123, 150, 178, 205}, {116, 142, 169, 195}, {111, 135, 160, 185}, {105, 128, 152, 175}, {100, 122, 144, 166},
  { 95, 116, 137, 158}, { 90, 110, 130, 150}, { 85, 104, 123, 142}, { 81,  99, 117, 135}, { 77,  94, 111, 128}, { 73,  89, 105, 122}, { 69,  85, 100, 116}, { 66,  80,  95, 110},
  { 62,  76,  90, 104}, { 59,  72,  86,  99}, { 56,  69,  81,  94}, { 53,  65,  77,  89}, { 51,  62,  73,  85}, { 48,  59,  69,  80}, { 46,  56,  66,  76}, { 43,  53,  63,  72},
  { 41,  50,  59,  69}, { 39,  48,  56,  65}, { 37,  45,  54,  62}, { 35,  43,  51,  59}, { 33,  41,  48,  56}, { 32,  39,  46,  53}, { 30,  37,  43,  50}, { 29,  35,  41,  48},
  { 27,  33,  39,  45}, { 26,  31,  37,  43}, { 24,  30,  35,  41}, { 23,  28,  33,  39}, { 22,  27,  32,  37}, { 21,  26,  30,  35}, { 20,  24,  29,  33}, { 19,  23,  27,  31},
  { 18,  22,  26,  30}, { 17,  21,  25,  28}, { 16,  20,  23,  27}, { 15,  19,  22,  25}, { 14,  18,  21,  24}, { 14,  17,  20,  23}, { 13,  16,  19,  22}, { 12,  15,  18,  21},
  { 12,  14,  17,  20}, { 11,  14,  16,  19}, { 11,  13,  15,  18}, { 10,  12,  15,  17}, { 10,  12,  14,  16}, {  9,  11,  13,  15}, {  9,  11,  12,  14}, {  8,  10,  12,  14},
  {  8,   9,  11,  13}, {  7,   9,  11,  12}, {  7,   9,  10,  12}, {  7,   8,  10,  11}, {  6,   8,   9,  11}, {  6,   7,   9,  10}, {  6,   7,   8,   9}, {  2,   2,   2,   2} };
static const uint8_t e_renorm_table[32] = { 6, 5, 4, 4, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1 };  /* cabac.c:84-88 */

static void ec_start(ecabac_t *c) { c->low = 0; c->range = 510; c->bits_left = 23; c->num_buffered_bytes = 0; c->buffered_byte = 0xff; }  /* cabac.c:90-99 */
static void ec_write(ecabac_t *c)  /* cabac.c:138-168 kvz_cabac_write */
{
  const uint32_t lead_byte = c->low >> (24 - c->bits_left);
  c->bits_left += 8;
  c->low &= 0xffffffffu >> c->bits_left;
  if (lead_byte == 0xff) { c->num_buffered_bytes++; return; }
  if (c->num_buffered_bytes > 0) {
    const uint32_t carry = lead_byte >> 8;
    uint32_t byte = c->buffered_byte + carry;
    c->buffered_byte = lead_byte & 0xff;
    eb_put_byte(c->out, byte);
    byte = (0xff + carry) & 0xff;
    while (c->num_buffered_bytes > 1) { eb_put_byte(c->out, byte); c->num_buffered_bytes--; }
  } else {
    c->num_buffered_bytes = 1;
    c->buffered_byte = lead_byte;
  }
}
static void ec_record(ecabac_t *c, uint32_t r) { if (c->rec_n < c->rec_cap) c->rec[c->rec_n] = r; c->rec_n++; }
static void ec_bin(ecabac_t *c, int idx, int bin)  /* cabac.c:104-133 kvz_cabac_encode_bin on context idx */
{
  if (c->rec) { ec_record(c, (uint32_t)idx | ((bin ? 1u : 0u) << 8)); return; }
  uint8_t *st = &c->ctx[idx];
  const uint32_t lps = e_lps_table[*st >> 1][(c->range >> 6) & 3];
  c->range -= lps;
  if ((bin ? 1 : 0) != (*st & 1)) {
    const int num_bits = e_renorm_table[lps >> 3];
    c->low = (c->low + c->range) << num_bits;
    c->range = lps << num_bits;
    *st = g_next_lps[*st];
    c->bits_left -= num_bits;
  } else {
    *st = g_next_mps[*st];
    if (c->range >= 256) return;
    c->low <<= 1;
    c->range <<= 1;
    c->bits_left--;
  }
  if (c->bits_left < 12) ec_write(c);
}
static void ec_ep(ecabac_t *c, uint32_t bin_values, int num_bins)  /* cabac.c:231-254 kvz_cabac_encode_bins_ep (a single bin: :215-226, the same arithmetic) */
{
  if (c->rec) {  /* 16 bins per record, most significant first */
    while (num_bins > 16) { num_bins -= 16; ec_record(c, 0x40000000u | (16u << 16) | ((bin_values >> num_bins) & 0xffffu)); bin_values &= (1u << num_bins) - 1; }
    if (num_bins > 0) ec_record(c, 0x40000000u | ((uint32_t)num_bins << 16) | (bin_values & 0xffffu));
    return;
  }
  while (num_bins > 8) {
    num_bins -= 8;
    const uint32_t pattern = bin_values >> num_bins;
    c->low <<= 8;
    c->low += c->range * pattern;
    bin_values -= pattern << num_bins;
    c->bits_left -= 8;
    if (c->bits_left < 12) ec_write(c);
  }
  c->low <<= num_bins;
  c->low += c->range * bin_values;
  c->bits_left -= num_bins;
  if (c->bits_left < 12) ec_write(c);
}
static void ec_trm(ecabac_t *c, int bin)  /* cabac.c:193-210 kvz_cabac_encode_bin_trm */
{
  c->range -= 2;
  if (bin) { c->low += c->range; c->low <<= 7; c->range = 2 << 7; c->bits_left -= 7; }
  else if (c->range >= 256) return;
  else { c->low <<= 1; c->range <<= 1; c->bits_left--; }
  if (c->bits_left < 12) ec_write(c);
}
static void ec_finish(ecabac_t *c)  /* cabac.c:170-191 kvz_cabac_finish */
{
  if (c->low >> (32 - c->bits_left)) {
    eb_put_byte(c->out, c->buffered_byte + 1);
    while (c->num_buffered_bytes > 1) { eb_put_byte(c->out, 0); c->num_buffered_bytes--; }
    c->low -= 1u << (32 - c->bits_left);
  } else {
    if (c->num_buffered_bytes > 0) eb_put_byte(c->out, c->buffered_byte);
    while (c->num_buffered_bytes > 1) { eb_put_byte(c->out, 0xff); c->num_buffered_bytes--; }
  }
  eb_put(c->out, c->low >> 8, 24 - c->bits_left);
}

/* ---- the residual coder in real mode (encode_coding_tree-generic.c:40-283; transform skip and encryption off; sign data hiding by `signhide`: a group whose first and
 * last levels lie four scan positions or more apart leaves out the sign coded last, :199 and :240-247) ---- */
static void e_last_xy(ecabac_t *c, int lastpos_x, int lastpos_y, int width, int type, int scan)  /* encode_coding_tree.c:63-115 */
{
  static const uint8_t min_in_group[10] = { 0, 1, 2, 3, 4, 6, 8, 12, 16, 24 };  /* encoderstate.h:393 g_min_in_group */
  int index = 0;
  while ((4 << index) < width) index++;
  const int ctx_offset = type ? 0 : (index * 3 + (index + 1) / 4), shift = type ? index : (index + 3) / 4;
  const int base_x = type ? CX_LAST_X_CHROMA : CX_LAST_X_LUMA, base_y = type ? CX_LAST_Y_CHROMA : CX_LAST_Y_LUMA;
  if (scan == 2) { const int tmp = lastpos_x; lastpos_x = lastpos_y; lastpos_y = tmp; }
  const int gx = g_group_idx[lastpos_x], gy = g_group_idx[lastpos_y];
  for (int i = 0; i < gx; i++) ec_bin(c, base_x + ctx_offset + (i >> shift), 1);
  if (gx < g_group_idx[width - 1]) ec_bin(c, base_x + ctx_offset + (gx >> shift), 0);
  for (int i = 0; i < gy; i++) ec_bin(c, base_y + ctx_offset + (i >> shift), 1);
  if (gy < g_group_idx[width - 1]) ec_bin(c, base_y + ctx_offset + (gy >> shift), 0);
  if (gx > 3) ec_ep(c, (uint32_t)(lastpos_x - min_in_group[gx]), (gx - 2) / 2);
  if (gy > 3) ec_ep(c, (uint32_t)(lastpos_y - min_in_group[gy]), (gy - 2) / 2);
}
static void e_coeff_remain(ecabac_t *c, uint32_t symbol, uint32_t r_param)  /* cabac.c:275-301 kvz_cabac_write_coeff_remain */
{
  int32_t code_number = (int32_t)symbol;
  uint32_t length;
  if (code_number < (3 << r_param)) {
    length = (uint32_t)code_number >> r_param;
    ec_ep(c, (1u << (length + 1)) - 2, (int)length + 1);
    ec_ep(c, (uint32_t)code_number % (1u << r_param), (int)r_param);
  } else {
    length = r_param;
    code_number -= 3 << r_param;
    while (code_number >= (1 << length)) { code_number -= 1 << length; ++length; }
    ec_ep(c, (1u << (3 + length + 1 - r_param)) - 2, (int)(3 + length + 1 - r_param));
    ec_ep(c, (uint32_t)code_number, (int)length);
  }
}
static void e_coeff_nxn(ecabac_t *c, const int16_t *coeff, int width, int type, int scan_mode, int signhide)
{
  int log2_size = 2;
  while ((1 << log2_size) < width) log2_size++;
  const int num_blk_side = width >> 2;
  const uint32_t *scan = kvz_oracle_scan_table(scan_mode, log2_size);
  static const uint32_t one_cg[1] = { 0 };
  uint32_t diag8[64];
  const uint32_t *scan_cg = log2_size == 2 ? one_cg : kvz_oracle_scan_table(log2_size == 3 ? scan_mode : 0, log2_size - 2);  /* tables.h:84-89 g_sig_last_scan_cg */
  if (log2_size == 5) {
    int n = 0;
    for (int d = 0; d < 15; d++) for (int x = 0; x <= d; x++) if (x < 8 && d - x < 8) diag8[n++] = (uint32_t)((d - x) * 8 + x);
    scan_cg = diag8;
  }
  uint8_t sig_cg[64] = { 0 };
  for (int cy = 0; cy < num_blk_side; cy++)
    for (int cx = 0; cx < num_blk_side; cx++)
      for (int i = 0; i < 16; i++) if (coeff[(cy * 4 + (i >> 2)) * width + cx * 4 + (i & 3)]) { sig_cg[cy * num_blk_side + cx] = 1; break; }
  int scan_cg_last = num_blk_side * num_blk_side - 1;
  while (!sig_cg[scan_cg[scan_cg_last]]) scan_cg_last--;
  int scan_pos_last = scan_cg_last * 16 + 15;
  while (!coeff[scan[scan_pos_last]]) scan_pos_last--;
  const int pos_last = (int)scan[scan_pos_last];
  e_last_xy(c, pos_last & (width - 1), pos_last >> log2_size, width, type, scan_mode);
  const int base_sig = type == 0 ? CX_SIG_LUMA : CX_SIG_CHROMA;
  int scan_pos_sig = scan_pos_last, c1 = 1;
  for (int i = scan_cg_last; i >= 0; i--) {
    const int sub_pos = i << 4, cg_blk_pos = (int)scan_cg[i], cg_pos_y = cg_blk_pos / num_blk_side, cg_pos_x = cg_blk_pos - cg_pos_y * num_blk_side;
    int abs_coeff[16], num_non_zero = 0;
    uint32_t coeff_signs = 0, go_rice = 0;
    int last_nz_pos_in_cg = -1, first_nz_pos_in_cg = 16;
    if (scan_pos_sig == scan_pos_last) { abs_coeff[0] = abs(coeff[pos_last]); coeff_signs = coeff[pos_last] < 0; num_non_zero = 1; last_nz_pos_in_cg = first_nz_pos_in_cg = scan_pos_sig; scan_pos_sig--; }
    const int right = cg_pos_x < num_blk_side - 1 && sig_cg[cg_pos_y * num_blk_side + cg_pos_x + 1];
    const int lower = cg_pos_y < num_blk_side - 1 && sig_cg[(cg_pos_y + 1) * num_blk_side + cg_pos_x];
    if (i == scan_cg_last || i == 0) sig_cg[cg_blk_pos] = 1;
    else ec_bin(c, CX_SIG_CG + type + (right || lower), sig_cg[cg_blk_pos]);  /* coded_sub_block_flag, context.c:315-327 */
    if (sig_cg[cg_blk_pos]) {
      const int pattern = width == 4 ? -1 : right + (lower << 1);  /* context.c:339-351 */
      for (; scan_pos_sig >= sub_pos; scan_pos_sig--) {
        const int blk_pos = (int)scan[scan_pos_sig], pos_y = blk_pos >> log2_size, pos_x = blk_pos - (pos_y << log2_size), sig = coeff[blk_pos] != 0;
        if (scan_pos_sig > sub_pos || i == 0 || num_non_zero) ec_bin(c, base_sig + sig_ctx_inc(pattern, scan_mode, pos_x, pos_y, log2_size, type), sig);
        if (sig) {
          abs_coeff[num_non_zero++] = abs(coeff[blk_pos]); coeff_signs = 2 * coeff_signs + (coeff[blk_pos] < 0);
          if (last_nz_pos_in_cg == -1) last_nz_pos_in_cg = scan_pos_sig;
          first_nz_pos_in_cg = scan_pos_sig;
        }
      }
    } else scan_pos_sig = sub_pos - 1;
    if (num_non_zero > 0) {
      int ctx_set = (i > 0 && type == 0) ? 2 : 0;
      if (c1 == 0) ctx_set++;
      c1 = 1;
      const int base_one = (type == 0 ? CX_ONE_LUMA : CX_ONE_CHROMA) + 4 * ctx_set, num_c1 = num_non_zero < 8 ? num_non_zero : 8;
      int first_c2 = -1;
      for (int idx = 0; idx < num_c1; idx++) {
        const int symbol = abs_coeff[idx] > 1;
        ec_bin(c, base_one + c1, symbol);
        if (symbol) { c1 = 0; if (first_c2 == -1) first_c2 = idx; }
        else if (c1 < 3 && c1 > 0) c1++;
      }
      if (c1 == 0 && first_c2 != -1) ec_bin(c, (type == 0 ? CX_ABS_LUMA : CX_ABS_CHROMA) + ctx_set, abs_coeff[first_c2] > 2);
      if (signhide && last_nz_pos_in_cg - first_nz_pos_in_cg >= 4) ec_ep(c, coeff_signs >> 1, num_non_zero - 1);
      else ec_ep(c, coeff_signs, num_non_zero);
      if (c1 == 0 || num_non_zero > 8) {
        int first_coeff2 = 1;
        for (int idx = 0; idx < num_non_zero; idx++) {
          const int base_level = idx < 8 ? 2 + first_coeff2 : 1;
          if (abs_coeff[idx] >= base_level) {
            e_coeff_remain(c, (uint32_t)(abs_coeff[idx] - base_level), go_rice);
            if (abs_coeff[idx] > 3 * (1 << go_rice)) go_rice = go_rice + 1 < 4 ? go_rice + 1 : 4;
          }
          if (abs_coeff[idx] >= 2) first_coeff2 = 0;
        }
      }
    }
  }
}

/* ---- the picture as the CTU pass returns it ---- */
typedef struct {
  int W, H, w8, w4;
  const uint8_t *depth, *mode, *part, *mode4;  /* per 8x8: CU depth, luma mode, NxN flag (or NULL); per 4x4: luma mode of NxN CUs (or NULL) */
  const int16_t *coeff;                          /* KVZ_HIP_CTU_COEFFS per CTU, raster CTU order; inside: Y | U | V, z-order */
  const int16_t *ctu;                            /* the current CTU's */
  int signhide;                                  /* the picture is coded with sign data hiding (kvz_hip_intra_cost_model::signhide) */
} epic_t;
static int e_any(const int16_t *c, int n) { for (int i = 0; i < n; i++) if (c[i]) return 1; return 0; }
static int e_mode_at(const epic_t *p, int x, int y)
{
  if (p->part && p->part[(y >> 3) * p->w8 + (x >> 3)]) return p->mode4[(y >> 2) * p->w4 + (x >> 2)];
  return p->mode[(y >> 3) * p->w8 + (x >> 3)];
}
/* coded block flag of the transform block of plane c whose luma origin is (x, y) (LCU-local) at tree depth `depth`: cbf_is_set(cu->cbf, depth, c) -- "any level of the
 * block or of the blocks below it" (cu.h:510-569) -- read off the levels themselves */
static int e_cbf(const epic_t *p, int c, int xl, int yl, int depth)
{
  const int w = 64 >> depth;
  if (c == 0) return e_any(p->ctu + zorder(xl, yl), w * w);
  const int cw = depth >= 3 ? 4 : w / 2;  /* the 8x8 CU's chroma blocks are 4x4 whatever the luma split */
  return e_any(p->ctu + (c == 1 ? 4096 : 5120) + zorder((xl & ~7) / 2, (yl & ~7) / 2), cw * cw);
}

static void e_transform_tree(ecabac_t *c, const epic_t *p, int x, int y, int depth, int tr_depth, int cu_tr_depth, int parent_u, int parent_v)  /* encode_coding_tree.c:193-310 */
{
  const int xl = x & 63, yl = y & 63;
  const int split = cu_tr_depth > depth;
  const int cb_y = e_cbf(p, 0, xl, yl, depth), cb_u = e_cbf(p, 1, xl, yl, depth), cb_v = e_cbf(p, 2, xl, yl, depth);
  /* split_transform_flag is never coded: tr_depth_intra 0; the 64x64 split and the NxN split are inferred (:236-243) */
  if (depth < 4) {
    if (tr_depth == 0 || parent_u) ec_bin(c, CX_CBF_CHROMA + tr_depth, cb_u);
    if (tr_depth == 0 || parent_v) ec_bin(c, CX_CBF_CHROMA + tr_depth, cb_v);
  }
  if (split) {
    const int o = 64 >> (depth + 1);
    e_transform_tree(c, p, x, y, depth + 1, tr_depth + 1, cu_tr_depth, cb_u, cb_v);
    e_transform_tree(c, p, x + o, y, depth + 1, tr_depth + 1, cu_tr_depth, cb_u, cb_v);
    e_transform_tree(c, p, x, y + o, depth + 1, tr_depth + 1, cu_tr_depth, cb_u, cb_v);
    e_transform_tree(c, p, x + o, y + o, depth + 1, tr_depth + 1, cu_tr_depth, cb_u, cb_v);
    return;
  }
  ec_bin(c, CX_CBF_LUMA + !tr_depth, cb_y);
  /* depth 4: the chroma flags are the 8x8 CU's (signalled one level up) */
  const int cu_u = depth == 4 ? parent_u : cb_u, cu_v = depth == 4 ? parent_v : cb_v;
  if (!(cb_y | cu_u | cu_v)) return;
  /* encode_transform_unit (:117-190) */
  const int w = 64 >> depth, cw = depth == 4 ? w : w / 2;
  if (cb_y) e_coeff_nxn(c, p->ctu + zorder(xl, yl), w, 0, scan_order(e_mode_at(p, x, y), depth), p->signhide);
  if (depth == 4 && (x % 8 == 0 || y % 8 == 0)) return;  /* the 4x4 chroma blocks follow the last luma block, under the first PU's mode */
  const int cscan = scan_order(e_mode_at(p, x & ~7, y & ~7), depth), cxl = (xl & ~7) / 2, cyl = (yl & ~7) / 2;
  if (cu_u) e_coeff_nxn(c, p->ctu + 4096 + zorder(cxl, cyl), cw, 2, cscan, p->signhide);
  if (cu_v) e_coeff_nxn(c, p->ctu + 5120 + zorder(cxl, cyl), cw, 2, cscan, p->signhide);
}

static void e_coding_tree(ecabac_t *c, const epic_t *p, int x, int y, int depth)  /* encode_coding_tree.c:745-900, I slice */
{
  const int w = 64 >> depth, half = w / 2;
  const int cur_depth = p->depth[(y >> 3) * p->w8 + (x >> 3)];
  const int split_flag = cur_depth > depth;
  const int border_x = p->W < x + w, border_y = p->H < y + w, border = border_x || border_y;
  const int border_split_x = p->W >= x + 8 + half, border_split_y = p->H >= y + 8 + half;
  if (depth != 3) {
    if (!border) {
      int sm = 0;
      if (x > 0 && p->depth[(y >> 3) * p->w8 + ((x - 1) >> 3)] > depth) sm++;
      if (y > 0 && p->depth[((y - 1) >> 3) * p->w8 + (x >> 3)] > depth) sm++;
      ec_bin(c, CX_SPLIT + sm, split_flag);
    }
    if (split_flag || border) {
      e_coding_tree(c, p, x, y, depth + 1);
      if (!border_x || border_split_x) e_coding_tree(c, p, x + half, y, depth + 1);
      if (!border_y || border_split_y) e_coding_tree(c, p, x, y + half, depth + 1);
      if (!border || (border_split_x && border_split_y)) e_coding_tree(c, p, x + half, y + half, depth + 1);
      return;
    }
  }
  const int nxn = depth == 3 && p->part && p->part[(y >> 3) * p->w8 + (x >> 3)];
  if (depth == 3) ec_bin(c, CX_PART, !nxn);  /* kvz_encode_part_mode :654-672 */
  /* encode_intra_coding_unit (:467-652): all prev_intra_luma_pred_flags, then per PU mpm_idx or rem_intra_luma_pred_mode, then the chroma mode (= the luma mode: "4") */
  const int n_pu = nxn ? 4 : 1;
  int8_t preds[4][3];
  int mpm[4], modes[4];
  for (int j = 0; j < n_pu; j++) {
    const int px = x + 4 * (j & 1), py = y + 4 * (j >> 1);
    cu_t lc = { 1, 0, 0, 0, 0 }, ac = { 1, 0, 0, 0, 0 }, *left = NULL, *above = NULL;
    modes[j] = e_mode_at(p, px, py);
    if (px > 0) { lc.mode = (uint8_t)e_mode_at(p, px - 1, py); left = &lc; }
    if (py % 64 > 0 && py > 0) { ac.mode = (uint8_t)e_mode_at(p, px, py - 1); above = &ac; }
    mpm_candidates(py, left, above, preds[j]);
    mpm[j] = -1;
    for (int i = 0; i < 3; i++) if (preds[j][i] == modes[j]) { mpm[j] = i; break; }
  }
  for (int j = 0; j < n_pu; j++) ec_bin(c, CX_INTRA, mpm[j] != -1);
  for (int j = 0; j < n_pu; j++) {
    if (mpm[j] != -1) {
      ec_ep(c, mpm[j] == 0 ? 0 : 1, 1);
      if (mpm[j] != 0) ec_ep(c, mpm[j] == 1 ? 0 : 1, 1);
    } else {
      int8_t *q = preds[j], tmp;
      if (q[0] > q[1]) { tmp = q[0]; q[0] = q[1]; q[1] = tmp; }
      if (q[0] > q[2]) { tmp = q[0]; q[0] = q[2]; q[2] = tmp; }
      if (q[1] > q[2]) { tmp = q[1]; q[1] = q[2]; q[2] = tmp; }
      int rem = modes[j];
      for (int i = 2; i >= 0; i--) rem = rem > q[i] ? rem - 1 : rem;
      ec_ep(c, (uint32_t)rem, 5);
    }
  }
  ec_bin(c, CX_CHROMA, 0);
  e_transform_tree(c, p, x, y, depth, 0, nxn ? 4 : (depth ? depth : 1), 0, 0);
}

static void e_sao_color(ecabac_t *c, const kvz_hip_sao_params *sao, int color)  /* encoderstate.c:467-517 encode_sao_color */
{
  const int off = color == 2 ? 5 : 0;
  if (color != 2) {
    ec_bin(c, KVZ_HIP_CX_SAO_TYPE, sao->type != 0);
    if (sao->type == 1) ec_ep(c, 0, 1); else if (sao->type == 2) ec_ep(c, 1, 1);
  }
  if (sao->type == 0) return;
  for (int i = 1; i <= 4; i++) {  /* cabac.c:526-551 kvz_cabac_write_unary_max_symbol_ep, max 7 */
    unsigned symbol = (unsigned)abs(sao->offsets[i + off]);
    const int code_last = 7 > symbol;
    ec_ep(c, symbol ? 1 : 0, 1);
    if (!symbol) continue;
    while (--symbol) ec_ep(c, 1, 1);
    if (code_last) ec_ep(c, 0, 1);
  }
  if (sao->type == 1) {
    for (int i = 1; i <= 4; i++) if (sao->offsets[i + off] != 0) ec_ep(c, sao->offsets[i + off] < 0 ? 1 : 0, 1);
    ec_ep(c, (uint32_t)sao->band_position[color == 2 ? 1 : 0], 5);
  } else if (color != 2) {
    ec_ep(c, (uint32_t)sao->eo_class, 2);
  }
}

/* (kvz_oracle.h declares both entry points) */
/* The slice data of one I picture: one substream per CTU row with WPP, one for the picture without.  m: qp, ctx_init (the slice's initial context states), no_wpp and signhide
 * are read.  cu_depth / cu_mode per 8x8, part / mode4 (or NULL) as kvz_hip_batch_download / _download_partitions return them; coeff as kvz_hip_batch_download returns it;
 * sao_luma / sao_chroma / sao_merge (or NULL when SAO is off): one record per LCU, merge 0 none / 1 left / 2 up.  out receives the substreams back to back,
 * substream_bytes their sizes; returns the total size (the caller checks it against capacity). */
size_t kvz_oracle_entropy_intra_picture(const kvz_hip_intra_cost_model *m, int width, int height, const uint8_t *cu_depth, const uint8_t *cu_mode, const uint8_t *part,
                                        const uint8_t *mode4, const int16_t *coeff, const kvz_hip_sao_params *sao_luma, const kvz_hip_sao_params *sao_chroma,
                                        const uint8_t *sao_merge, uint8_t *out, size_t capacity, uint32_t *substream_bytes)
{
  return kvz_oracle_entropy_intra_tile(m, width, height, cu_depth, cu_mode, part, mode4, coeff, sao_luma, sao_chroma, sao_merge, 0, out, capacity, substream_bytes);
}
/* ... of a tile: not_last != 0 when other tiles of the slice follow (the tile then ends in end_of_subset_one_bit, encoderstate.c:699-724) */
size_t kvz_oracle_entropy_intra_tile(const kvz_hip_intra_cost_model *m, int width, int height, const uint8_t *cu_depth, const uint8_t *cu_mode, const uint8_t *part,
                                     const uint8_t *mode4, const int16_t *coeff, const kvz_hip_sao_params *sao_luma, const kvz_hip_sao_params *sao_chroma,
                                     const uint8_t *sao_merge, int not_last, uint8_t *out, size_t capacity, uint32_t *substream_bytes)
{
  build_transitions();
  const int wc = (width + 63) / 64, hc = (height + 63) / 64;
  epic_t p = { width, height, width >> 3, width >> 2, cu_depth, cu_mode, part, mode4, coeff, NULL, m->signhide != 0 };
  ebits_t bits = { out, capacity, 0, 0, 0, 0, 0 };
  ecabac_t c, next_row;
  memset(&c, 0, sizeof c);
  c.out = &bits;
  memcpy(c.ctx, m->ctx_init, KVZ_HIP_CX_SAO_TYPE + 1);
  next_row = c;
  ec_start(&c);
  for (int ly = 0; ly < hc; ly++) {
    const size_t begin = bits.n;
    if (!m->no_wpp && ly > 0) { memcpy(c.ctx, next_row.ctx, sizeof c.ctx); }  /* encoderstate.c:763-771: the contexts after the second LCU of the row above */
    for (int lx = 0; lx < wc; lx++) {
      p.ctu = coeff + (size_t)(ly * wc + lx) * KVZ_HIP_CTU_COEFFS;
      if (sao_luma) {  /* encoderstate.c:519-552 encode_sao */
        const int merge = sao_merge[ly * wc + lx];
        if (lx > 0) ec_bin(&c, KVZ_HIP_CX_SAO_MERGE, merge == 1);
        if (ly > 0 && merge != 1) ec_bin(&c, KVZ_HIP_CX_SAO_MERGE, merge == 2);
        if (!merge) { e_sao_color(&c, &sao_luma[ly * wc + lx], 0); e_sao_color(&c, &sao_chroma[ly * wc + lx], 1); e_sao_color(&c, &sao_chroma[ly * wc + lx], 2); }
      }
      e_coding_tree(&c, &p, lx * 64, ly * 64, 0);
      const int last_col = lx == wc - 1, last_row = ly == hc - 1, end_of_slice = last_col && last_row && !not_last;
      ec_trm(&c, end_of_slice);  /* end_of_slice_segment_flag (:699-712) */
      if ((last_col && last_row) || (!m->no_wpp && last_col)) {
        if (!end_of_slice) ec_trm(&c, 1);  /* end_of_subset_one_bit */
        ec_finish(&c);
        eb_put(&bits, 1, 1);
        eb_align_zero(&bits);
        bits.zerocount = 0;  /* the next substream is a bitstream_t of its own (one per leaf encoder state) */
        ec_start(&c);
      }
      if (!m->no_wpp && lx == 1) memcpy(next_row.ctx, c.ctx, sizeof c.ctx);
    }
    if (!m->no_wpp) substream_bytes[ly] = (uint32_t)(bits.n - begin);
  }
  if (m->no_wpp) substream_bytes[0] = (uint32_t)bits.n;
  return bits.n;
}

/* ---- the per-call form (strategies-encode.h:49-65): one transform block ---- */
/* the block's bins as records (include/kvz_hip.h kvz_hip_coeff_nxn_bins); returns their number */
int kvz_oracle_coeff_nxn_bins(const int16_t *coeff, int width, int type, int scan_mode, uint32_t *records, int capacity)
{
  ecabac_t c;
  memset(&c, 0, sizeof c);
  c.rec = records; c.rec_cap = capacity;
  e_coeff_nxn(&c, coeff, width, type, scan_mode, 0);
  return c.rec_n;
}
/* `n` records through the arithmetic coder, contexts starting from ctx_states (KVZ_HIP_CX_* order), then the coder's flush, a stop bit and the alignment: the bytes
 * kvz_encode_coeff_nxn + kvz_cabac_finish leave in the stream for that block.  Returns the number of bytes. */
int kvz_oracle_code_records(const uint8_t *ctx_states, const uint32_t *records, int n, uint8_t *out, int capacity)
{
  build_transitions();
  ebits_t bits = { out, (size_t)capacity, 0, 0, 0, 0, 0 };
  ecabac_t c;
  memset(&c, 0, sizeof c);
  c.out = &bits;
  memcpy(c.ctx, ctx_states, KVZ_HIP_CX_SAO_TYPE + 1);
  ec_start(&c);
  for (int i = 0; i < n; i++) {
    const uint32_t r = records[i];
    if ((r >> 30) == 0) ec_bin(&c, (int)(r & 0xff), (int)((r >> 8) & 1));
    else if ((r >> 30) == 1) ec_ep(&c, r & 0xffff, (int)((r >> 16) & 0x3f));
    else ec_trm(&c, (int)(r & 1));
  }
  ec_finish(&c);
  eb_put(&bits, 1, 1);
  eb_align_zero(&bits);
  return (int)bits.n;
}

/* ---- B pictures of a low-delay sequence (kvz_oracle_inter.inc): kvz_encode_coding_tree with the inter syntax (encode_coding_tree.c:745-900, kvz_encode_inter_prediction_unit
 * :311-421, kvz_encode_mvd :1062-1112, cabac.c:556-586 kvz_cabac_write_ep_ex_golomb), one reference picture per list, 2Nx2N CUs, max_merge 5 ---- */
static void eb_merge_idx(ecabac_t *c, int merge_idx)
{
  for (int ui = 0; ui < 4; ui++) {
    const int symbol = ui != merge_idx;
    if (ui == 0) ec_bin(c, CXB_MERGE_IDX, symbol); else ec_ep(c, (uint32_t)symbol, 1);
    if (!symbol) break;
  }
}
static void eb_ex_golomb(ecabac_t *c, uint32_t symbol, uint32_t count)
{
  uint32_t bins = 0;
  int num_bins = 0;
  while (symbol >= (1u << count)) { bins = 2 * bins + 1; ++num_bins; symbol -= 1u << count; ++count; }
  bins = 2 * bins; ++num_bins;
  bins = (bins << count) | symbol;
  num_bins += (int)count;
  ec_ep(c, bins, num_bins);
}
static void eb_mvd(ecabac_t *c, int hor, int ver)
{
  const uint32_t ah = (uint32_t)abs(hor), av = (uint32_t)abs(ver);
  ec_bin(c, CXB_MVD, hor != 0);
  ec_bin(c, CXB_MVD, ver != 0);
  if (hor) ec_bin(c, CXB_MVD + 1, ah > 1);
  if (ver) ec_bin(c, CXB_MVD + 1, av > 1);
  if (hor) { if (ah > 1) eb_ex_golomb(c, ah - 2, 1); ec_ep(c, hor > 0 ? 0 : 1, 1); }
  if (ver) { if (av > 1) eb_ex_golomb(c, av - 2, 1); ec_ep(c, ver > 0 ? 0 : 1, 1); }
}
static void eb_coding_tree(ecabac_t *c, ctu_t *t, int x, int y, int depth)
{
  const int w = LCU >> depth, half = w / 2, w4 = t->W >> 2;
  const cu_t *cur = &t->fcu[(y >> 2) * w4 + (x >> 2)];
  const int split_flag = cur->depth > depth;
  const int border_x = t->W < x + w, border_y = t->H < y + w, border = border_x || border_y;
  const int border_split_x = t->W >= x + 8 + half, border_split_y = t->H >= y + 8 + half;
  level_t *l0 = &t->lv[0];
  if (depth != 3) {
    if (!border) ec_bin(c, CX_SPLIT + split_model(t, l0, x, y, depth), split_flag);
    if (split_flag || border) {
      eb_coding_tree(c, t, x, y, depth + 1);
      if (!border_x || border_split_x) eb_coding_tree(c, t, x + half, y, depth + 1);
      if (!border_y || border_split_y) eb_coding_tree(c, t, x, y + half, depth + 1);
      if (!border || (border_split_x && border_split_y)) eb_coding_tree(c, t, x + half, y + half, depth + 1);
      return;
    }
  }
  ec_bin(c, CXB_SKIP + skip_context(t, l0, x, y), cur->skipped);
  if (cur->skipped) { eb_merge_idx(c, cur->merge_idx); return; }
  ec_bin(c, CXB_PRED_MODE, cur->type == 1);
  if (cur->type == 2 || depth == 3) ec_bin(c, CX_PART, 1);  /* 2Nx2N */
  const int xl = x - t->cx, yl = y - t->cy, cw = depth == 3 ? 4 : w / 2;
  const int cb_y = cbf_is_set(cur->cbf, depth, 0), cb_u = cbf_is_set(cur->cbf, depth, 1), cb_v = cbf_is_set(cur->cbf, depth, 2);
  int scan = 0;
  if (cur->type == 2) {
    ec_bin(c, CXB_MERGE_FLAG, cur->merged);
    if (cur->merged) eb_merge_idx(c, cur->merge_idx);
    else {
      const int inter_dir = cur->mv_dir - 1;
      ec_bin(c, CXB_INTER_DIR + depth, inter_dir == 2);
      if (inter_dir < 2) ec_bin(c, CXB_INTER_DIR + 4, inter_dir);
      for (int l = 0; l < 2; l++) {
        if (!(cur->mv_dir & (1 << l))) continue;
        int16_t mv_cand[2][2];
        mv_candidates(t, l0, x, y, w, w, l, mv_cand);
        const int k = cur->mv_cand[l];
        eb_mvd(c, cur->mv[l][0] - mv_cand[k][0], cur->mv[l][1] - mv_cand[k][1]);
        ec_bin(c, CXB_MVP_IDX, k);  /* kvz_cabac_write_unary_max_symbol, max_symbol 1 */
      }
    }
    const int cbf = cbf_is_set_any(cur->cbf, depth);
    if (!cur->merged) ec_bin(c, CXB_ROOT_CBF, cbf);
    if (!cbf) return;
    ec_bin(c, CX_CBF_CHROMA, cb_u);
    ec_bin(c, CX_CBF_CHROMA, cb_v);
    if (cb_u || cb_v) ec_bin(c, CX_CBF_LUMA + 1, cb_y);  /* else inferred 1 (encode_coding_tree.c:276-279) */
  } else {
    cu_t lc, ac, *left = NULL, *above = NULL;
    if (x > 0 && neighbour_cu(t, l0, x - 1, y, &lc)) left = &lc;
    if (y % LCU > 0 && y > 0 && neighbour_cu(t, l0, x, y - 1, &ac)) above = &ac;
    int8_t preds[3];
    mpm_candidates(y, left, above, preds);
    int mpm = -1;
    for (int i = 2; i >= 0; i--) if (preds[i] == cur->mode) mpm = i;
    ec_bin(c, CX_INTRA, mpm != -1);
    if (mpm != -1) { ec_ep(c, mpm == 0 ? 0 : 1, 1); if (mpm != 0) ec_ep(c, mpm == 1 ? 0 : 1, 1); }
    else {
      int8_t tmp;
      if (preds[0] > preds[1]) { tmp = preds[0]; preds[0] = preds[1]; preds[1] = tmp; }
      if (preds[0] > preds[2]) { tmp = preds[0]; preds[0] = preds[2]; preds[2] = tmp; }
      if (preds[1] > preds[2]) { tmp = preds[1]; preds[1] = preds[2]; preds[2] = tmp; }
      int rem = cur->mode;
      for (int i = 2; i >= 0; i--) rem = rem > preds[i] ? rem - 1 : rem;
      ec_ep(c, (uint32_t)rem, 5);
    }
    ec_bin(c, CX_CHROMA, 0);
    ec_bin(c, CX_CBF_CHROMA, cb_u);
    ec_bin(c, CX_CBF_CHROMA, cb_v);
    ec_bin(c, CX_CBF_LUMA + 1, cb_y);
    scan = scan_order(cur->mode, depth);
  }
  if (cb_y) e_coeff_nxn(c, &l0->coeff[0][zorder(xl, yl)], w, 0, scan, 0);  /* (B pictures never hide signs: the inter pass has no hiding step) */
  if (cb_u) e_coeff_nxn(c, &l0->coeff[1][zorder(xl / 2, yl / 2)], cw, 2, scan, 0);
  if (cb_v) e_coeff_nxn(c, &l0->coeff[2][zorder(xl / 2, yl / 2)], cw, 2, scan, 0);
}

/* the slice data of one B picture after its search: t as b_picture left it (fcu, in); coeff: KVZ_HIP_CTU_COEFFS per CTU; init: the slice's initial context states (CX_ALL) */
static size_t e_b_picture(ctu_t *t, const uint8_t *init, int no_wpp, const int16_t *coeff, const kvz_hip_sao_params *sao_luma, const kvz_hip_sao_params *sao_chroma,
                          const uint8_t *sao_merge, uint8_t *out, size_t capacity, uint32_t *substream_bytes)
{
  const int wc = (t->W + 63) / 64, hc = (t->H + 63) / 64, w4 = t->W >> 2;
  ebits_t bits = { out, capacity, 0, 0, 0, 0, 0 };
  ecabac_t c, next_row;
  memset(&c, 0, sizeof c);
  c.out = &bits;
  memcpy(c.ctx, init, CX_ALL);
  next_row = c;
  ec_start(&c);
  for (int ly = 0; ly < hc; ly++) {
    const size_t begin = bits.n;
    if (!no_wpp && ly > 0) memcpy(c.ctx, next_row.ctx, sizeof c.ctx);
    for (int lx = 0; lx < wc; lx++) {
      /* the CTU's level-0 work tree as the search left it: CU records and levels (what mv_candidates / the transform tree read inside the CTU) */
      t->cx = lx * 64; t->cy = ly * 64;
      level_t *l0 = &t->lv[0];
      for (int yy = 0; yy < 64 && t->cy + yy < t->H; yy += 4)
        for (int xx = 0; xx < 64 && t->cx + xx < t->W; xx += 4) *cu_at(l0, xx, yy) = t->fcu[((t->cy + yy) >> 2) * w4 + ((t->cx + xx) >> 2)];
      const int16_t *cc = coeff + (size_t)(ly * wc + lx) * KVZ_HIP_CTU_COEFFS;
      memcpy(l0->coeff[0], cc, 4096 * sizeof(int16_t)); memcpy(l0->coeff[1], cc + 4096, 1024 * sizeof(int16_t)); memcpy(l0->coeff[2], cc + 5120, 1024 * sizeof(int16_t));
      if (sao_luma) {
        const int merge = sao_merge[ly * wc + lx];
        if (lx > 0) ec_bin(&c, KVZ_HIP_CX_SAO_MERGE, merge == 1);
        if (ly > 0 && merge != 1) ec_bin(&c, KVZ_HIP_CX_SAO_MERGE, merge == 2);
        if (!merge) { e_sao_color(&c, &sao_luma[ly * wc + lx], 0); e_sao_color(&c, &sao_chroma[ly * wc + lx], 1); e_sao_color(&c, &sao_chroma[ly * wc + lx], 2); }
      }
      eb_coding_tree(&c, t, lx * 64, ly * 64, 0);
      const int last_col = lx == wc - 1, last_row = ly == hc - 1, end_of_slice = last_col && last_row;
      ec_trm(&c, end_of_slice);
      if ((last_col && last_row) || (!no_wpp && last_col)) {
        if (!end_of_slice) ec_trm(&c, 1);
        ec_finish(&c);
        eb_put(&bits, 1, 1);
        eb_align_zero(&bits);
        bits.zerocount = 0;
        ec_start(&c);
      }
      if (!no_wpp && lx == 1) memcpy(next_row.ctx, c.ctx, sizeof c.ctx);
    }
    if (!no_wpp) substream_bytes[ly] = (uint32_t)(bits.n - begin);
  }
  if (no_wpp) substream_bytes[0] = (uint32_t)bits.n;
  return bits.n;
}

/* The slice data of one B picture from its CU records alone (kvz_oracle.h): the ctu_t as b_picture leaves it -- the picture's records, the reference picture's for the
 * temporal MV predictors (which exist from POC 2 on, inter.c:1290), the B slice's initial states -- handed to e_b_picture.  No search runs: records that a coder can
 * walk are the caller's business (every 4x4 unit of a CU carries the CU's record, skipped implies merged, a coded block flag is set exactly when its block has a level). */
size_t kvz_oracle_entropy_b_picture(int qp, int poc, int no_wpp, int width, int height, const kvz_oracle_cu *cu, const kvz_oracle_cu *ref_cu, const int16_t *coeff,
                                    const kvz_hip_sao_params *sao_luma, const kvz_hip_sao_params *sao_chroma, const uint8_t *sao_merge, uint8_t *out, size_t capacity,
                                    uint32_t *substream_bytes)
{
  build_transitions();
  ctu_t *t = (ctu_t *)calloc(1, sizeof(ctu_t));
  kvz_hip_intra_cost_model m;
  struct inter_seq in;
  uint8_t init[CX_ALL];
  memset(&m, 0, sizeof m);
  memset(&in, 0, sizeof in);
  b_slice_contexts(qp, init);
  m.qp = qp; m.no_wpp = no_wpp;
  in.poc = poc; in.ref_cu = ref_cu;
  in.ref[0] = (const uint8_t *)ref_cu;  /* mv_candidates only asks whether a reference picture exists; no sample is read */
  t->m = &m; t->W = width; t->H = height; t->fcu = (cu_t *)cu; t->slice_b = 1; t->in = &in;
  build_avail_tables(t);
  const size_t n = e_b_picture(t, init, no_wpp, coeff, sao_luma, sao_chroma, sao_merge, out, capacity, substream_bytes);
  free(t);
  return n;
}
