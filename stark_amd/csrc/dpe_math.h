// The semiparametric density-product sampler's arithmetic: ONE definition for k_dpe_img (dpe.hip) and its
// host twin (stk_dpe_sample_host).  Every product-sum is an explicit fma and contraction is off, so the
// device and the host round the same operations in the same order ("density product").
//
// Philox counters (stream < 2^24 rides in the tag word, c3 = stream << 8 | TAG):
//   TAG_DPE_INIT  ctr = {chain, m >> 2, 0, c3}   initial index of coordinate m: 32-bit word m & 3
//                                               (r.a low, r.a high, r.b low, r.b high), index = mulhi(word, S)
//   TAG_DPE_PROP  ctr = {chain, sweep, m, c3}    proposal of (chain, sweep, m): index = mulhi(r.a low, S),
//                                               uniform = u53(r.b); accept iff log(uniform) < log W' - log W
//   TAG_DPE_NORM  ctr = {chain, j, i >> 1, c3}   Box-Muller normals of coordinates i, i ^ 1 of the chain's
//                                               j-th emitted draw
// Every number is drawn whether or not it decides anything.
//
// State of a chain: the indices t[M], s = sum_m y^m_{t_m} (coordinate j in lane j & 63, slot j >> 6),
// N = sum_m n^m_{t_m}, G = sum_m g^m_{t_m}, q = ||s||^2.  A proposal (m, c) moves them as
//   s' = (s - y^m_{t_m}) + y^m_c,   N' = (N - n_old) + n_new,   G' = (G - g_old) + g_new
// and q' = ||s'||^2 is the lane partial sums (slots in order, fma) added by the xor butterfly 32, 16 .. 1,
// which leaves the same bits in every lane.
//   log W = -(N - q / M) a - q b + G,   a = 1 / (2 h^2),   b = 1 / (2 M (1 + h^2))
//   y     = s ms + sd z,                ms = 1 / (M (1 + h^2)),   sd = sqrt(h^2 / (M (1 + h^2)))
// (a, b, ms, sd) of every sweep come from the host (dpe_coef): no device pow, division or sqrt.
#pragma once
#include <math.h>
#include <stdint.h>
#include "philox.h"

#pragma clang fp contract(off)

namespace stk {

constexpr int DPE_MAX_P = 1024;                  // 16 coordinates per lane
constexpr int DPE_MAX_NC = 16;
constexpr int DPE_MAX_SHARDS = 4096;             // the chain's indices and accept counts live in LDS
constexpr uint32_t DPE_MAX_STREAM = 1u << 24;

struct DpeCoef { double a, b, ms, sd; };

__host__ __device__ constexpr int dpe_ldp(int p) { return (p + 7) & ~7; }   // row stride of the image: whole 64-B lines

inline DpeCoef dpe_coef(double h, int M) {
  const double h2 = h * h, d = (double)M * (1.0 + h2);
  return DpeCoef{1.0 / (2.0 * h2), 1.0 / (2.0 * d), 1.0 / d, sqrt(h2 / d)};
}

STK_HD uint32_t dpe_c3(uint32_t tag, uint32_t stream) { return (stream << 8) | tag; }
STK_HD uint32_t dpe_mulhi(uint32_t word, uint32_t S) { return (uint32_t)(((uint64_t)word * S) >> 32); }

STK_HD uint32_t dpe_init_index(uint64_t seed, uint32_t stream, uint32_t chain, uint32_t m, uint32_t S) {
  const u64x2 r = philox(seed, chain, m >> 2, 0, dpe_c3(TAG_DPE_INIT, stream));
  const uint64_t w = (m & 2) ? r.b : r.a;
  return dpe_mulhi((m & 1) ? (uint32_t)(w >> 32) : (uint32_t)w, S);
}

struct DpeProposal { uint32_t c; double logu; };
STK_HD DpeProposal dpe_proposal(uint64_t seed, uint32_t stream, uint32_t chain, uint32_t sweep, uint32_t m, uint32_t S) {
  const u64x2 r = philox(seed, chain, sweep, m, dpe_c3(TAG_DPE_PROP, stream));
  return DpeProposal{dpe_mulhi((uint32_t)r.a, S), log(u53(r.b))};
}

STK_HD double dpe_normal(uint64_t seed, uint32_t stream, uint32_t chain, uint32_t draw, uint32_t coord) {
  return normal_at(seed, chain, draw, 0, coord, dpe_c3(TAG_DPE_NORM, stream));
}

STK_HD double dpe_move(double cur, double old_v, double new_v) { return (cur - old_v) + new_v; }

STK_HD double dpe_logw(double N, double q, double G, double inv_m, const DpeCoef& c) {
  const double t = fma(-q, inv_m, N);
  return fma(-t, c.a, fma(-q, c.b, G));
}

STK_HD double dpe_draw(double s, double z, const DpeCoef& c) { return fma(c.sd, z, s * c.ms); }

// the host's butterfly over the 64 lane partial sums (part is overwritten)
inline double dpe_butterfly_host(double part[64]) {
  double tmp[64];
  for (int o = 32; o > 0; o >>= 1) {
    for (int l = 0; l < 64; ++l) tmp[l] = part[l] + part[l ^ o];
    for (int l = 0; l < 64; ++l) part[l] = tmp[l];
  }
  return part[0];
}

}  // namespace stk
