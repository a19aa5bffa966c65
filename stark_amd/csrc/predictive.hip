// The pointwise log-predictive sweep (regression families, 1 <= d <= 128): for every ROW of a shard,
// statistics over S posterior draws of the row's normalised log likelihood -- the reduction the
// sampler's sweeps never form (they reduce over rows for each draw).  No reference counterpart: it is
// what WAIC, the log pointwise predictive density and the fitted mean are made of (DESIGN.md
// sections 3 and 8; the definitions are in include/stark_hip.h).  The forward pass -- the draw image
// that k_predictive_prep lays out here, eta, ll and g -- is draw_forward.h's.
//
//   per row   lppd = logsumexp_s ll - log S, mean = sum ll / S, var = sample variance of ll (0 at S = 1),
//             mu = sum g / S
//
// k_predictive: workgroup = 4 waves, two workgroups per CU, chunks of whole 64-row groups; wave w of a
// block owns rows 16 w .. 16 w + 15 of the group, and the four waves share every draw-tile slab through
// the slab ring (the same LDS area as the rows' slots, once the rows are in registers).  Per draw tile
// the wave evaluates ll and g on the MFMA output registers and updates, per row, a streaming state:
//   m, s      running maximum and scaled sum of the logsumexp: a draw with ll = -inf adds 0 and never
//             meets -inf - -inf; a new maximum rescales s by exp(-(ll - m));
//   a, b      sum (ll - c) and sum (ll - c)^2 about the shift c = the row's ll at draw 0 (0 where that is
//             not finite): the cancellation in b - a^2 / S costs (mean - c)^2 eps <= 4 scale^2 eps;
//             a -inf draw makes a = -inf and b = +inf, so mean = -inf and var = inf - inf = NaN as the
//             definitions give them, and a NaN stays NaN;
//   gs        sum g.
// A fixed-order xor butterfly over the 16 draw lanes ends each row; the logsumexp joins the lanes'
// (m, s) pairs at the common maximum.  The per-row log and lgamma are the library's.
// Row i's statistics depend only on (x_i, y_i) and the draws.
#include "draw_forward.h"
#include <algorithm>

namespace stk {

constexpr int PD_R = 16;          // rows per wave tile = MFMA M
constexpr int PD_W = 4;           // waves per block
constexpr int PD_GPC = 4;         // 64-row groups per chunk before the chunk count saturates
constexpr int PD_GMAX = 256;      // chunks per shard at most

__host__ __device__ inline int pred_chunks(int64_t n) { return draw_chunks(draw_units(n, PD_R * PD_W), PD_GPC, PD_GMAX); }
// the exp table, then ONE area that holds the four waves' rows while a group starts and the slab ring after
__host__ __device__ constexpr size_t pred_lds_doubles(int d) {
  const size_t ring = (size_t)2 * pred_slab(pred_kf(d)), rows = (size_t)PD_W * PD_R * d;
  return EX_TAB + (ring > rows ? ring : rows);
}

struct PrepArgs {
  const double* q;          // [S][D]
  double* img;
  int family, d, D, S, ntile;
};

__global__ __launch_bounds__(256) void k_predictive_prep(PrepArgs A) {
  const int kf = pred_kf(A.d), slab = pred_slab(kf);
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)A.ntile * slab) return;
  const int t = (int)(idx / slab), r = (int)(idx - (int64_t)t * slab);
  double v = 0.0;
  if (r >= kf * 64 + 64) {
    // padding of the slab
  } else if (r < kf * 64) {
    const int s = r >> 6, lane = r & 63, lg = lane >> 4, lr = lane & 15;
    const int col = 4 * s + lg, draw = 16 * t + lr;
    if (draw < A.S && col < A.d) v = A.q[(size_t)draw * A.D + 1 + col];
  } else {
    const int j = r - kf * 64, kind = j >> 4, draw = 16 * t + (j & 15);
    if (draw < A.S) {
      const double u = A.family == STK_LINREG ? A.q[(size_t)draw * A.D + A.d + 1] : 0.0;
      v = kind == 0 ? A.q[(size_t)draw * A.D] : (kind == 1 ? u : (kind == 2 ? exp(-2.0 * u) : 1.0));
    }
  }
  A.img[idx] = v;
}

template <int FAM, int KF>
__global__ __launch_bounds__(64 * PD_W, 2) void k_predictive(PredArgs A) {
  constexpr double NINF = -__builtin_huge_val();
  const int si = blockIdx.y, chunk = blockIdx.x;
  const ShardDev sh = A.shards[A.shard0 + si];
  const int G = pred_chunks(sh.n);
  if (chunk >= G) return;                            // block-uniform
  const int d = sh.d, S = A.S;
  const int tid = threadIdx.x, lane = tid & 63, w = uniform_int(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4;

  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* const tab = lds;                           // [EX_TAB] 2^(j/1024)
  double* const ring = lds + EX_TAB;                 // [2][SLAB] draw-tile slabs
  double* const xs = ring + (size_t)w * PD_R * d;    // [16][d] the wave's rows, before the ring is filled
  exp_table_init(tab);

  const UnitRange groups = draw_chunk_units(draw_units(sh.n, PD_R * PD_W), chunk, G);
  const gptr_t<double> xg = gp(sh.x);
  SlabRing<KF, PD_W> slabs{ring, gp(A.img), tid};
  const int64_t lim = sh.n * d;
  const double dS = (double)S, logS = log(dS);
  double tot[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};    // sum lppd, var, elpd, elpd^2, #var > 0.4, #non-finite

  for (int64_t grp = groups.first; grp < groups.last; ++grp) {
    const int64_t row0 = grp * (PD_R * PD_W) + w * PD_R;
    double yv[4], lgam[4];
    draw_row_y<FAM, true>(sh, row0, lr, lg, yv, lgam);
    __builtin_amdgcn_sched_barrier(0);               // lgamma is done before the rows take their registers
    // ---- the wave's 16 rows into the A registers
    draw_stage_rows(xs, xg, row0 * d, lim, d, lane, 64);
    __syncthreads();
    double a[KF];
    draw_load_a<KF>(xs, d, lr, lg, a);
    __syncthreads();                                 // every wave has its rows: the area becomes the ring
    slabs.fill_first();
    __syncthreads();

    double m[4], sc[4], sa[4], sb[4], gs[4], sft[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      m[i] = NINF;
      sc[i] = sa[i] = sb[i] = gs[i] = sft[i] = 0.0;
    }
#pragma nounroll                                      // and no peeling of tile 0: one copy of the body
    for (int t = 0; t < A.ntile; ++t) {
      const double* B = slabs.slab(t);
      const double alpha = B[KF * 64 + lr], u = B[KF * 64 + 16 + lr], e2u = B[KF * 64 + 32 + lr];
      const bool live = B[KF * 64 + 48 + lr] != 0.0;
      const dbl4 eta4 = draw_eta<KF>(a, B, alpha, lane);
      __builtin_amdgcn_sched_barrier(0);
      // the next slab, into registers while the statistics run (the B operands' registers are free now)
      if (t + 1 < A.ntile) slabs.prefetch(t + 1);
      double ll[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double g;
        ll[i] = draw_ll<FAM>(eta4[i], yv[i], lgam[i], u, e2u, tab, g);
        if (!live) g = 0.0;
        gs[i] += g;
      }
      // the shift: the row's ll at draw 0 (lane lr = 0 of tile 0), 0 where it is not finite
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double c = __shfl(ll[i], lane & 48);
        sft[i] = t != 0 ? sft[i] : (isfinite(c) ? c : 0.0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double dl = live ? ll[i] - sft[i] : 0.0;
        sa[i] += dl;
        sb[i] = fma(dl, dl, sb[i]);
        // logsumexp: ll = -inf (and a padding draw) adds 0; a NaN is caught through sa
        const double lv = live ? ll[i] : NINF;
        const double df = lv - m[i];                 // NaN only for -inf - -inf or a NaN ll
        const bool skip = !(lv > NINF);              // -inf or NaN
        const double ex = skip ? 0.0 : pd_exp(-fabs(df), tab);
        const bool up = !skip && df > 0.0;
        sc[i] = up ? fma(sc[i], ex, 1.0) : sc[i] + ex;
        m[i] = up ? lv : m[i];
      }
      if (t + 1 < A.ntile) slabs.commit(t + 1);
      __syncthreads();
    }

    // ---- the 16 draw lanes of every row, in a fixed order
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double M = m[i];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const double v = __shfl_xor(M, o);
        M = v > M ? v : M;
      }
      double sl = m[i] > NINF ? sc[i] * pd_exp(m[i] - M, tab) : 0.0;
      double va = sa[i], vb = sb[i], vg = gs[i];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        sl += __shfl_xor(sl, o);
        va += __shfl_xor(va, o);
        vb += __shfl_xor(vb, o);
        vg += __shfl_xor(vg, o);
      }
      double lppd = M > NINF ? M + log(sl) - logS : NINF;
      if (va != va) lppd = va;                       // a NaN draw
      const double mean = sft[i] + va / dS;
      double var = va != va ? va : 0.0;              // S = 1: 0 by definition, NaN for a NaN draw
      if (S > 1) {
        var = (vb - va * va / dS) / (dS - 1.0);
        var = var < 0.0 ? 0.0 : var;                 // rounding only; a NaN stays
      }
      const double mu = vg / dS;
      const int64_t row = row0 + lg + 4 * i;
      if (row < sh.n) {
        const double elpd = lppd - var;
        tot[0] += lppd;
        tot[1] += var;
        tot[2] += elpd;
        tot[3] = fma(elpd, elpd, tot[3]);
        tot[4] += var > 0.4 ? 1.0 : 0.0;
        tot[5] += (isfinite(lppd) && isfinite(mean) && isfinite(var) && isfinite(mu)) ? 0.0 : 1.0;
        if (A.rows && lr < 4) {
          const double v = lr == 0 ? lppd : (lr == 1 ? mean : (lr == 2 ? var : mu));
          A.rows[(A.rowoff[si] + row) * 4 + lr] = v;
        }
      }
      __builtin_amdgcn_sched_barrier(0);             // one row group at a time: four interleaved logs spill
    }
  }

  // ---- block totals: lanes lr = 0 hold their rows' sums; (wave, lane group) order
  __syncthreads();
  double* red = ring;                                // [PD_W][4][6]
  if (lr == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) red[(w * 4 + lg) * 6 + k] = tot[k];
  }
  __syncthreads();
  if (tid < 6) {
    double v = 0.0;
    for (int j = 0; j < PD_W * 4; ++j) v += red[j * 6 + tid];
    A.partial[((size_t)si * A.Gs + chunk) * 8 + tid] = v;
  }
}

template <int FAM, int KF>
static hipError_t go_predictive(const PredArgs& A, int d, int nsh, hipStream_t st) {
  const size_t lds = pred_lds_doubles(d) * sizeof(double);
  auto kern = k_predictive<FAM, KF>;
  if (lds > 64 * 1024)
    if (const hipError_t e = allow_big_lds(reinterpret_cast<const void*>(kern))) return e;
  hipLaunchKernelGGL(kern, dim3(A.Gs, nsh), dim3(64 * PD_W), lds, st, A);
  return hipGetLastError();
}

}  // namespace stk

using namespace stk;

bool stk_predictive_supported(int d) { return d >= 1 && d <= 128; }
int stk_predictive_chunks(int64_t n) { return pred_chunks(n); }
int stk_predictive_rows_per_tile() { return PD_R; }
int stk_predictive_waves() { return PD_W; }
int stk_predictive_tiles(int S) { return (S + 15) / 16; }
size_t stk_predictive_lds_bytes(int d) { return pred_lds_doubles(d) * sizeof(double); }
size_t stk_predictive_image_bytes(int d, int S) {
  return sizeof(double) * (size_t)stk_predictive_tiles(S) * pred_slab(pred_kf(d));
}
size_t stk_predictive_ws_bytes(int64_t n) { return sizeof(double) * 8 * (size_t)pred_chunks(n); }

// q [S][D] -> the draw image (stk_predictive_image_bytes)
hipError_t stk_launch_predictive_prep(int family, int d, int D, int S, const double* q, double* img, hipStream_t st) {
  const PrepArgs A{q, img, family, d, D, S, stk_predictive_tiles(S)};
  const int64_t n = (int64_t)A.ntile * pred_slab(pred_kf(d));
  hipLaunchKernelGGL(k_predictive_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A);
  return hipGetLastError();
}

// Shards [shard0, shard0 + nsh) against the image -> totals [nsh][8] and, unless rows is null, the
// per-row statistics at rowoff[s] (device array of nsh offsets); partial holds nsh * Gs chunks of 8
// doubles, Gs >= every shard's chunk count.  One sweep launch and one reduce launch for all of them.
hipError_t stk_launch_predictive(int family, const ShardDev* shards, int shard0, int nsh, int d, int Gs, int S,
                                 const double* img, double* partial, double* rows, const int64_t* rowoff,
                                 double* totals, hipStream_t st) {
  const PredArgs A{shards, img, partial, rows, rowoff, totals, family, shard0, Gs, S, stk_predictive_tiles(S)};
  const hipError_t e = draw_dispatch(family, d, [&](auto fam, auto kf) {
    return go_predictive<decltype(fam)::value, decltype(kf)::value>(A, d, nsh, st);
  });
  return e != hipSuccess ? e : launch_draw_totals<pred_chunks, 6>(A, nsh, st);   // [7] = 0
}
