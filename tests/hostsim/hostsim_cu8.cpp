// hostsim_cu8.cpp -- TEST INFRASTRUCTURE.  Stages 2-5 of the 8x8 CU's reconstruction on blocks without a picture around them, serially: the functions of
// kvz_recon.hpp that kvz_ctu.hpp recon_cu8 and the device entry point kvz_hip_dev_cu8_units call (cu8_matrix_rows, cu8_fwd_first / _second, cu8_inv_first / _second,
// cu8_transposed: the arithmetic, the row a lane reads, its matrix rows, the transposed index), compiled for the host, one "lane" after the other per stage.  What is
// restated here is only what recon_cu8 itself keeps: which buffer a stage reads and writes.  Same arguments as kvz_hip_dev_cu8_units (include/kvz_hip_dev.h).
// tests/test_cu8_blocks.py builds it and holds both against the per-call oracle's dct -> quant -> dequant -> idct at inputs no picture reaches.
#define KVZ_HOSTSIM 1
#include "../../kvazaar_amd/csrc/kvz_recon.hpp"
#include "../../kvazaar_amd/csrc/kvz_tables.hpp"

namespace {
struct MatRow { uint32_t w[4]; };
template <int L2> void plane(const kvz::Tables *tb, int type, int qp, int from_coeffs, const int16_t *in, int16_t *levels, int16_t *dequant, int16_t *resid)
{
  constexpr int nn = 1 << (2 * L2);
  alignas(16) int16_t t0[nn], t1[nn];
  MatRow fwd[nn] = {}, inv[nn] = {};
  const kvz::QuantScalars q = kvz::quant_scalars(qp, 8, 1, 0, 1 << L2, type);
  for (int e = 0; e < nn; e++) { kvz::cu8_matrix_rows<L2>(tb, e, fwd[e], inv[e]); if (!from_coeffs) t0[e] = in[e]; }                       // stage 1: the residual
  for (int e = 0; e < nn && !from_coeffs; e++) t1[e] = kvz::cu8_fwd_first<L2>(t0, e, fwd[e]);                                             // stage 2
  for (int e = 0; e < nn; e++) {                                                                                                          // stage 3
    int level = 0, dq = in[e];
    if (!from_coeffs) { level = kvz::quant_level(kvz::cu8_fwd_second<L2>(t1, e, fwd[e]), q); dq = kvz::dequant_level(level, q); }
    levels[e] = (int16_t)level;
    dequant[e] = (int16_t)dq;
    t0[kvz::cu8_transposed<L2>(e)] = (int16_t)dq;
  }
  for (int e = 0; e < nn; e++) t1[kvz::cu8_transposed<L2>(e)] = kvz::cu8_inv_first<L2>(t0, e, inv[e]);                                    // stage 4
  for (int e = 0; e < nn; e++) resid[e] = kvz::cu8_inv_second<L2>(t1, e, inv[e]);                                                         // stage 5
}
}  // namespace

extern "C" int kvz_hostsim_cu8_units(int count, int from_coeffs, const int16_t *in, const int32_t *qp, int16_t *levels, int16_t *dequant, int16_t *resid)
{
  static kvz::Tables tb;
  kvz::build_tables(&tb);
  if (count < 0 || (from_coeffs != 0 && from_coeffs != 1)) return -1;
  for (int u = 0; u < count; u++) {
    const long o = 96l * u;
    plane<3>(&tb, 0, qp[u], from_coeffs, in + o, levels + o, dequant + o, resid + o);
    plane<2>(&tb, 2, qp[u], from_coeffs, in + o + 64, levels + o + 64, dequant + o + 64, resid + o + 64);
    plane<2>(&tb, 2, qp[u], from_coeffs, in + o + 80, levels + o + 80, dequant + o + 80, resid + o + 80);
  }
  return 0;
}
