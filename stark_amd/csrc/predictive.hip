// The pointwise log-predictive sweep (regression families, 1 <= d <= 128): for every ROW of a shard,
// statistics over S posterior draws of the row's normalised log likelihood -- the reduction the
// sampler's sweeps never form (they reduce over rows for each draw).  No reference counterpart: it is
// what WAIC, the log pointwise predictive density and the fitted mean are made of (DESIGN.md
// sections 3 and 8; the definitions are in include/stark_hip.h).
//
//   eta_is = alpha_s + x_i . beta_s           the forward half of a 16-chain sweep, for S draws
//   logistic  z = (2 y_i - 1) eta, ll = min(z, 0) - log1p(exp(-|z|)),          g = 1 / (1 + exp(-eta))
//   poisson   ll = y_i eta - exp(eta) - lgamma(y_i + 1),                       g = exp(eta)
//   linear    r = y_i - eta, ll = -log(2 pi)/2 - u_s - r^2 e^{-2 u_s} / 2,     g = eta
//   per row   lppd = logsumexp_s ll - log S, mean = sum ll / S, var = sample variance of ll (0 at S = 1),
//             mu = sum g / S
//
// k_predictive_prep lays the draws out as a K-major image of 16-draw tiles: tile t is one slab of
// KF = ceil(d / 4) k-steps x 64 lanes, lane (lr, lg) of k-step s holding beta_{16 t + lr}[4 s + lg]
// (the B operand of v_mfma_f64_16x16x4 as the lanes read it: one conflict-free ds_read_b64 per MFMA),
// then four rows of 16 per-draw scalars: alpha, u = log sigma, e^{-2u}, and 1 / 0 for a live / padding
// draw (the slab is padded to a multiple of 256 doubles, one block-wide copy).  Padding draws and columns are zero and masked out of every statistic.
//
// k_predictive: workgroup = 4 waves, two workgroups per CU.  A shard is cut into G chunks
// of whole 64-row groups that depend only on n; wave w of a block owns rows 16 w .. 16 w + 15 of the
// group and holds them as the A operand in registers for the whole draw loop (KF doubles per lane,
// read once from HBM, nontemporal, through a per-wave LDS slot so the global reads are contiguous).
// The four waves share every draw-tile slab through a two-slot LDS ring (the same LDS area, once the
// rows are in registers), filled one tile ahead through registers: the image leaves L2 once per block, not once per wave.  Per draw tile the wave forms
// eta[16 rows][16 draws] (lane (lr, lg): rows lg + 4 i of draw lr), evaluates ll and g on the MFMA
// output registers and updates, per row, a streaming state:
//   m, s      running maximum and scaled sum of the logsumexp: a draw with ll = -inf adds 0 and never
//             meets -inf - -inf; a new maximum rescales s by exp(-(ll - m));
//   a, b      sum (ll - c) and sum (ll - c)^2 about the shift c = the row's ll at draw 0 (0 where that is
//             not finite): the cancellation in b - a^2 / S costs (mean - c)^2 eps <= 4 scale^2 eps;
//             a -inf draw makes a = -inf and b = +inf, so mean = -inf and var = inf - inf = NaN as the
//             definitions give them, and a NaN stays NaN;
//   gs        sum g.
// A fixed-order xor butterfly over the 16 draw lanes ends each row; the logsumexp joins the lanes'
// (m, s) pairs at the common maximum.  The exponentials, the reciprocal and log1p of the hot loop are
// predictive_math.h's (table exp, ~2 ulp; a NaN is put back where the clamp of the exp would lose it);
// the per-row log and lgamma are the library's.
// Row i's statistics depend only on (x_i, y_i) and the draws.  Every chunk writes its partial totals;
// k_predictive_reduce sums them in chunk order, so the totals are bitwise independent of how many
// shards share a launch and of which GPU runs a shard.
#include "launchers.h"
#include "sweep_common.h"
#include "predictive_math.h"
#include <math.h>
#include <algorithm>

namespace stk {

constexpr int PD_R = 16;          // rows per wave tile = MFMA M
constexpr int PD_W = 4;           // waves per block
constexpr int PD_GPC = 4;         // 64-row groups per chunk before the chunk count saturates
constexpr int PD_GMAX = 256;      // chunks per shard at most

__host__ __device__ inline int pred_chunks(int64_t n) {
  const int64_t ng = (n + PD_R * PD_W - 1) / (PD_R * PD_W), g = (ng + PD_GPC - 1) / PD_GPC;
  return (int)(g < 1 ? 1 : (g > PD_GMAX ? PD_GMAX : g));
}
// the exp table, then ONE area that holds the four waves' rows while a group starts and the slab ring after
__host__ __device__ constexpr size_t pred_lds_doubles(int d) {
  const size_t ring = (size_t)2 * pred_slab(pred_kf(d)), rows = (size_t)PD_W * PD_R * d;
  return EX_TAB + (ring > rows ? ring : rows);
}

struct PredArgs {
  const ShardDev* shards;
  const double* img;        // [ntile][slab] the draw image
  double* partial;          // [nsh][Gs][8] chunk-partial totals
  double* rows;             // nullptr, or [sum n][4] (lppd, mean, var, mu), shard-major
  const int64_t* rowoff;    // [nsh] first row of every shard of the launch in `rows`
  double* totals;           // [nsh][8]
  int family, shard0, Gs, S, ntile;
};

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
  constexpr int SLAB = pred_slab(KF), NPF = SLAB / (64 * PD_W);
  constexpr double NINF = -__builtin_huge_val();
  const int si = blockIdx.y, chunk = blockIdx.x;
  const ShardDev sh = A.shards[A.shard0 + si];
  const int G = pred_chunks(sh.n);
  if (chunk >= G) return;                            // block-uniform
  const int d = sh.d, S = A.S;
  constexpr bool LIN = FAM == STK_LINREG, LOGI = FAM == STK_LOGREG, POIS = FAM == STK_POISSON;
  static_assert(LIN || LOGI || POIS, "k_predictive: unknown family");
  const int tid = threadIdx.x, lane = tid & 63, w = uniform_int(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4;

  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* const tab = lds;                           // [EX_TAB] 2^(j/1024)
  double* const ring = lds + EX_TAB;                 // [2][SLAB] draw-tile slabs
  double* const xs = ring + (size_t)w * PD_R * d;    // [16][d] the wave's rows, before the ring is filled
  exp_table_init(tab);

  const int64_t ng = (sh.n + PD_R * PD_W - 1) / (PD_R * PD_W);
  const int64_t g0 = ng * chunk / G, g1 = ng * (chunk + 1) / G;
  const gptr_t<double> xg = gp(sh.x);
  const gptr_t<double> img = gp(A.img);
  const int64_t lim = sh.n * d;
  const double dS = (double)S, logS = log(dS);
  double tot[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};    // sum lppd, var, elpd, elpd^2, #var > 0.4, #non-finite

  for (int64_t grp = g0; grp < g1; ++grp) {
    const int64_t row0 = grp * (PD_R * PD_W) + w * PD_R;
    // y of rows lg + 4 i; poisson: lgamma(y + 1) once per row (lane lr takes row lr) and handed round
    double yv[4], lgam[4], lgr = 0.0;
    if constexpr (POIS) {
      const int64_t row = row0 + lr;
      lgr = lgamma((row < sh.n ? (double)sh.yi[row] : 0.0) + 1.0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t row = row0 + lg + 4 * i;
      yv[i] = 0.0;
      if (row < sh.n) yv[i] = LIN ? sh.y[row] : (double)sh.yi[row];
      lgam[i] = POIS ? __shfl(lgr, lg + 4 * i) : 0.0;
    }
    __builtin_amdgcn_sched_barrier(0);               // lgamma is done before the rows take their registers
    // ---- the wave's 16 rows: contiguous in HBM, through the slot, into the A registers
    const int64_t base = row0 * d;
    for (int i = lane; i < PD_R * d; i += 64) xs[i] = base + i < lim ? __builtin_nontemporal_load(xg + base + i) : 0.0;
    __syncthreads();
    double a[KF];
#pragma unroll
    for (int s = 0; s < KF; ++s) {
      const int col = 4 * s + lg;
      a[s] = col < d ? xs[lr * d + col] : 0.0;
    }
    __syncthreads();                                 // every wave has its rows: the area becomes the ring
    double pf[NPF];
#pragma unroll
    for (int j = 0; j < NPF; ++j) {
      const int k = tid + 64 * PD_W * j;
      ring[k] = img[k];
    }
    __syncthreads();

    double m[4], sc[4], sa[4], sb[4], gs[4], sft[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      m[i] = NINF;
      sc[i] = sa[i] = sb[i] = gs[i] = sft[i] = 0.0;
    }
#pragma nounroll                                      // and no peeling of tile 0: one copy of the body
    for (int t = 0; t < A.ntile; ++t) {
      const double* B = ring + (t & 1) * SLAB;
      const double alpha = B[KF * 64 + lr], u = B[KF * 64 + 16 + lr], e2u = B[KF * 64 + 32 + lr];
      const bool live = B[KF * 64 + 48 + lr] != 0.0;
      dbl4 e0 = dbl4{alpha, alpha, alpha, alpha}, e1 = dbl4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < KF; ++s) {
        if (s & 1) e1 = mfma_f64(a[s], B[s * 64 + lane], e1);
        else e0 = mfma_f64(a[s], B[s * 64 + lane], e0);
        if ((s & 7) == 7) __builtin_amdgcn_sched_barrier(0);   // B reads at most 8 k-steps ahead: registers
      }
      const dbl4 eta4 = e0 + e1;
      __builtin_amdgcn_sched_barrier(0);
      // the next slab, into registers while the statistics run (the B operands' registers are free now)
      if (t + 1 < A.ntile) {
#pragma unroll
        for (int j = 0; j < NPF; ++j) {
          const int k = tid + 64 * PD_W * j;
          pf[j] = img[(size_t)(t + 1) * SLAB + k];
        }
      }
      double ll[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double eta = eta4[i];
        double g;
        if constexpr (LOGI) {
          const double z = yv[i] != 0.0 ? eta : -eta;
          const double e = pd_exp(-fabs(eta), tab);
          const double r1 = pd_rcp(1.0 + e);
          const double lt = (z < 0.0 ? z : 0.0) - pd_log1p01(e);
          ll[i] = eta != eta ? eta : lt;             // pd_exp turns a NaN into 0: put it back
          g = eta >= 0.0 ? r1 : e * r1;
          g = eta != eta ? eta : g;
        } else if constexpr (LIN) {
          const double r = yv[i] - eta;
          ll[i] = -0.91893853320467274178 - u - 0.5 * (r * r) * e2u;
          g = eta;
        } else {
          g = pd_exp(eta, tab);
          g = eta != eta ? eta : g;
          ll[i] = yv[i] * eta - g - lgam[i];
        }
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
      if (t + 1 < A.ntile) {
        double* Bn = ring + ((t + 1) & 1) * SLAB;
#pragma unroll
        for (int j = 0; j < NPF; ++j) {
          const int k = tid + 64 * PD_W * j;
          Bn[k] = pf[j];
        }
      }
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

// totals[s][1 + k] = the chunk partials of shard s summed in chunk order; [0] = n, [7] = 0
__global__ __launch_bounds__(64) void k_predictive_reduce(PredArgs A, int nsh) {
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= nsh * 8) return;
  const int si = idx >> 3, k = idx & 7;
  const ShardDev sh = A.shards[A.shard0 + si];
  double v = 0.0;
  if (k == 0) {
    v = (double)sh.n;
  } else if (k < 7) {
    const int G = pred_chunks(sh.n);
    const double* src = A.partial + (size_t)si * A.Gs * 8 + (k - 1);
    v = src[0];
    for (int c = 1; c < G; ++c) v += src[(size_t)c * 8];
  }
  A.totals[idx] = v;
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

template <int FAM>
static hipError_t launch_predictive(const PredArgs& A, int d, int nsh, hipStream_t st) {
  switch (pred_kf(d)) {
#define STK_PD(K) case K: return go_predictive<FAM, K>(A, d, nsh, st);
    STK_PD(1) STK_PD(2) STK_PD(3) STK_PD(4) STK_PD(5) STK_PD(6) STK_PD(7) STK_PD(8)
    STK_PD(9) STK_PD(10) STK_PD(11) STK_PD(12) STK_PD(13) STK_PD(14) STK_PD(15) STK_PD(16)
    STK_PD(17) STK_PD(18) STK_PD(19) STK_PD(20) STK_PD(21) STK_PD(22) STK_PD(23) STK_PD(24)
    STK_PD(25) STK_PD(26) STK_PD(27) STK_PD(28) STK_PD(29) STK_PD(30) STK_PD(31) STK_PD(32)
#undef STK_PD
  }
  return hipErrorInvalidValue;
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
  hipError_t e = hipErrorInvalidValue;
  if (family == STK_LOGREG) e = launch_predictive<STK_LOGREG>(A, d, nsh, st);
  else if (family == STK_LINREG) e = launch_predictive<STK_LINREG>(A, d, nsh, st);
  else if (family == STK_POISSON) e = launch_predictive<STK_POISSON>(A, d, nsh, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_predictive_reduce, dim3((nsh * 8 + 63) / 64), dim3(64), 0, st, A, nsh);
  return hipGetLastError();
}
