// hostsim_cu16_predict.cpp -- TEST INFRASTRUCTURE.  The serial host twin of kvz_hip_dev_cu16_predict (include/kvz_hip_dev.h): stage 1's luma prediction of a 16x16
// CU's reconstruction in the intra CTU pass (kvz_ctu.hpp recon_cu16) on reference sets without a picture around them.  The same functions the pass and the device
// entry point call -- the reference filter (luma_filtered_ref), the extended references (Tables::mref_tab, mref_copy), and the lane's row segment of four samples
// (kvz_recon.hpp cu16_predict_lane) -- compiled for the host, one "lane" after the other per stage, on a byte image laid out like CtuShared from its `ref` on.
// Same arguments and output as the device entry point.  tests/test_cu16_predict.py builds it and holds it against the oracle's intra prediction.
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
}  // namespace

// covered (may be null): 256 bytes per CU, +1 for every sample a lane wrote
extern "C" int kvz_hostsim_cu16_predict(const uint8_t *top, const uint8_t *left, const uint8_t *modes, int count, uint8_t *out, uint8_t *covered)
{
  if (count < 0) return -1;
  constexpr int W = 16, N = 2 * W + 1, NQ = 2 * W + 2;
  const kvz::Tables *tb = tables();
  for (long cu = 0; cu < count; cu++) {
    uint8_t img[kvz::kMrefExtended + 15 * kvz::kMrefStride + 16] = {};
    for (int k = 0; k < N; k++) { img[k] = top[cu * N + k]; img[kvz::kMrefRefRow + k] = left[cu * N + k]; }
    for (int i = 0; i < 2 * N; i++) img[kvz::kMrefFiltered + kvz::kMrefRefRow * (i >= N) + (i >= N ? i - N : i)] = kvz::luma_filtered_ref(img, N, i);
    for (int i = 0; i < 15 * NQ; i++) kvz::mref_copy<1>(img, &tb->mref_tab[1][i]);
    const int mode = kvz::imin(modes[cu], 34);
    int disp, inv;
    kvz::angular_params(mode, &disp, &inv);
    const int dc = kvz::dc_value(4, img, img + kvz::kMrefRefRow);
    for (int lane = 0; lane < 64; lane++) {
      uint8_t p[4];
      kvz::cu16_predict_lane(img, mode, dc, disp, inv, lane, p);
      const kvz::RowSegment g = kvz::cu16_luma_segment(lane);
      for (int k = 0; k < 4; k++) {
        out[cu * (W * W) + g.py * W + g.px0 + k] = p[k];
        if (covered) covered[cu * (W * W) + g.py * W + g.px0 + k]++;
      }
    }
  }
  return 0;
}
