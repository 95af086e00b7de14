// hostsim_satd_rows.cpp -- TEST INFRASTRUCTURE.  The rough search's row table (Tables::satd_rows, kvz_tables.hpp) and a scalar walk of it on reference sets
// without a picture around them: the functions of kvz_ops.hpp that kvz_ctu.hpp's rough search and the device entry point kvz_hip_dev_rough_rows call -- the
// reference filter (luma_filtered_ref), the extended references (Tables::mref_tab, mref_copy), the edge bytes of modes 10 / 26 (satd_edge_byte) -- compiled for the
// host, one "lane" after the other per stage, on a byte image laid out like CtuShared from its `ref` on; then every row of every (mode, block) pair by
// satd_row_walk, the scalar statement of what the device's packed row generator (kvz_mfma.hpp satd_rows_predict) makes of a table row.  Same arguments and output
// as kvz_hip_dev_rough_rows (include/kvz_hip_dev.h).  tests/test_satd_rows_table.py builds it and holds table and rows against the oracle's intra prediction.
#define KVZ_HOSTSIM 1
#include "../../kvazaar_amd/csrc/kvz_recon.hpp"
#include "../../kvazaar_amd/csrc/kvz_tables.hpp"

namespace {
const kvz::Tables *tables()
{
  static kvz::Tables tb;
  static bool built = false;
  if (!built) { kvz::build_tables(&tb); built = true; }
  return &tb;
}
template <int L2> void cu_rows(const kvz::Tables *tb, const uint8_t *top, const uint8_t *left, uint8_t *out)
{
  constexpr int W = 1 << L2, N = 2 * W + 1, NQ = 2 * W + 2, LB = 2 * (L2 - 3), NBLK = 1 << LB;
  uint8_t img[kvz::kSatdEdge + 1 + 2 * 16 + 16] = {};
  for (int k = 0; k < N; k++) { img[k] = top[k]; img[kvz::kMrefRefRow + k] = left[k]; }
  for (int i = 0; i < 2 * N; i++) img[kvz::kMrefFiltered + kvz::kMrefRefRow * (i >= N) + (i >= N ? i - N : i)] = kvz::luma_filtered_ref(img, N, i);
  for (int i = 0; i < 15 * NQ; i++) kvz::mref_copy<1>(img, &tb->mref_tab[L2 - 3][i]);
  img[kvz::kSatdEdge] = 0;
  for (int i = 0; i < 2 * W; i++) img[kvz::kSatdEdge + 1 + i] = kvz::satd_edge_byte(img, L2, i);
  for (int g = 0; g < (L2 == 4 ? 4 : 1); g++)
    for (int lane = 0; lane < 64; lane++) {
      const int pr = 32 * g + (lane & 31), mode = 2 + (pr >> LB), b = pr & (NBLK - 1);
      const uint32_t *e = tb->satd_rows[L2 == 4 ? 1 + g : 0][lane];
      uint8_t *o = out + ((mode - 2) * NBLK + b) * 64;
      for (int i = 0; i < 4; i++) {
        uint8_t v[8];
        kvz::satd_row_walk(img, e[2 * i], e[2 * i + 1], v);
        const int r = 4 * (lane >> 5) + i;
        for (int x = 0; x < 8; x++) o[mode >= 18 ? 8 * r + x : 8 * x + r] = v[x];
      }
    }
}
}  // namespace

// the table ([5][64][8] words) and the layout constants its entries are relative to: kMrefRefRow, kMrefFiltered, kMrefExtended, kMrefStride, kMrefOrg, kSatdSrcT,
// kSatdEdge, kSatdWindow, kSatdSrcVertical
extern "C" void kvz_hostsim_satd_rows_table(uint32_t *table, uint32_t *layout)
{
  memcpy(table, tables()->satd_rows, sizeof tables()->satd_rows);
  const uint32_t l[9] = { kvz::kMrefRefRow, kvz::kMrefFiltered, kvz::kMrefExtended, kvz::kMrefStride, kvz::kMrefOrg, kvz::kSatdSrcT, kvz::kSatdEdge, kvz::kSatdWindow, kvz::kSatdSrcVertical };
  memcpy(layout, l, sizeof l);
}

extern "C" int kvz_hostsim_rough_rows(int log2w, const uint8_t *top, const uint8_t *left, int count, uint8_t *out)
{
  if (count < 0 || (log2w != 3 && log2w != 4)) return -1;
  const int n = 2 * (1 << log2w) + 1, per = 32 * (log2w == 4 ? 4 : 1) * 64;
  for (long u = 0; u < count; u++) {
    if (log2w == 3) cu_rows<3>(tables(), top + u * n, left + u * n, out + u * per);
    else cu_rows<4>(tables(), top + u * n, left + u * n, out + u * per);
  }
  return 0;
}
