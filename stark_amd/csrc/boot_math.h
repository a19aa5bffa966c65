// The bootstrap weight w_ib of row i in replicate b: a pure function of (seed, stream, row, replicate),
// ONE definition for k_boot16 (boot.hip) and its host twin (stk_boot_weights_host).
//
//   counter  {(uint32)(i >> 4), ((uint32)(i >> 36) << 2) | (i & 3), stream << 12 | b, TAG_BOOT}
//            i: the row's index in its shard (int64), b < 4096, stream < 2^20 (the shard's global index)
//   words    r.a low, r.a high, r.b low, r.b high; row i takes word (i >> 2) & 3
// so the rows lh, lh + 4, lh + 8, lh + 12 (lh < 4) of a 16-row tile that starts at a multiple of 16 -- the
// four rows a lane of a 16x16x4 fp64 MFMA output holds -- are the four words of one Philox call.
//   kind 0 (poisson)      w = #{k : T_k <= word}, T_k = floor(2^32 sum_{j <= k} e^-1 / j!), k = 0 .. 12:
//                         integers 0 .. 13 with P(w = k) the Poisson(1) mass to within 2^-32
//   kind 1 (exponential)  w = -log((word + 1/2) 2^-32): Exp(1), mean 1, at most 22.9
#pragma once
#include <math.h>
#include <stdint.h>
#include "philox.h"

namespace stk {

constexpr int BOOT_POISSON = 0, BOOT_EXPONENTIAL = 1;
constexpr int BOOT_MAX_REPS = 4096;                 // b is 12 bits of the counter
constexpr uint32_t BOOT_MAX_STREAM = 1u << 20;      // stream is the other 20
constexpr int BOOT_NTHR = 13;

// the 13 thresholds, in increasing order
#define STK_BOOT_THRESHOLDS(X)                                                                             \
  X(0x5E2D58D8u) X(0xBC5AB1B1u) X(0xEB715E1Du) X(0xFB239797u) X(0xFF1025F5u) X(0xFFD90F3Bu) X(0xFFFA8B71u) \
  X(0xFFFF540Cu) X(0xFFFFED1Fu) X(0xFFFFFE21u) X(0xFFFFFFD4u) X(0xFFFFFFFCu) X(0xFFFFFFFFu)

STK_HD uint32_t boot_poisson(uint32_t word) {
  uint32_t w = 0;
#define STK_BOOT_COUNT(T) w += word >= T ? 1u : 0u;
  STK_BOOT_THRESHOLDS(STK_BOOT_COUNT)
#undef STK_BOOT_COUNT
  return w;
}

STK_HD double boot_exponential(uint32_t word) { return -log(((double)word + 0.5) * 0x1.0p-32); }

STK_HD double boot_weight_of_word(int kind, uint32_t word) {
  return kind == BOOT_POISSON ? (double)boot_poisson(word) : boot_exponential(word);
}

// the four words of the Philox call that serves row i (and the three other rows of its tile with i & 3
// and i >> 4 in common)
STK_HD void boot_words(uint64_t seed, uint32_t stream, int64_t row, uint32_t b, uint32_t out[4]) {
  const uint64_t i = (uint64_t)row;
  const u64x2 r = philox(seed, (uint32_t)(i >> 4), ((uint32_t)(i >> 36) << 2) | (uint32_t)(i & 3), (stream << 12) | b,
                         TAG_BOOT);
  out[0] = (uint32_t)r.a;
  out[1] = (uint32_t)(r.a >> 32);
  out[2] = (uint32_t)r.b;
  out[3] = (uint32_t)(r.b >> 32);
}

STK_HD double boot_weight(uint64_t seed, uint32_t stream, int64_t row, uint32_t b, int kind) {
  uint32_t wd[4];
  boot_words(seed, stream, row, b, wd);
  return boot_weight_of_word(kind, wd[(row >> 2) & 3]);
}

inline void boot_poisson_thresholds(uint32_t out[BOOT_NTHR]) {
  int k = 0;
#define STK_BOOT_STORE(T) out[k++] = T;
  STK_BOOT_THRESHOLDS(STK_BOOT_STORE)
#undef STK_BOOT_STORE
}

}  // namespace stk
