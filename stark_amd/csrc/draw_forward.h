// The forward pass that the sweeps over a DRAW IMAGE share (predictive.hip, loo.hip, logdens.hip): one
// definition of every piece, each kernel keeping its own loop structure and what it does with eta.
//
//   eta_is = alpha_s + x_i . beta_s           the forward half of a 16-chain sweep, for S draws
//   logistic  z = (2 y_i - 1) eta, ll = min(z, 0) - log1p(exp(-|z|)),          g = 1 / (1 + exp(-eta))
//   poisson   ll = y_i eta - exp(eta) - lgamma(y_i + 1),                       g = exp(eta)
//   linear    r = y_i - eta, ll = -log(2 pi)/2 - u_s - r^2 e^{-2 u_s} / 2,     g = eta
//
// k_predictive_prep (predictive.hip) lays the draws out as a K-major image of 16-draw tiles: tile t is one
// slab of KF = ceil(d / 4) k-steps x 64 lanes, lane (lr, lg) of k-step s holding beta_{16 t + lr}[4 s + lg]
// (the B operand of v_mfma_f64_16x16x4 as the lanes read it: one conflict-free ds_read_b64 per MFMA),
// then four rows of 16 per-draw scalars: alpha, u = log sigma, e^{-2u}, and 1 / 0 for a live / padding
// draw (the slab is padded to a multiple of 256 doubles, one block-wide copy).  Padding draws and
// columns are zero and masked out of every result.
//
// A shard is cut into G chunks of whole row units (64-row groups, or 16-row tiles) that depend only on n.
// A wave holds 16 rows as the A operand in registers for its whole draw loop (KF doubles per lane, read
// once from HBM, nontemporal, through an LDS slot so the global reads are contiguous) and forms, per
// draw tile, eta[16 rows][16 draws]: lane (lr, lg) has rows lg + 4 i of draw lr.  Where the waves of a
// block share every slab (SlabRing), it goes through a two-slot LDS ring filled one tile ahead through
// registers: the image leaves L2 once per block, not once per wave.  The exponentials, the reciprocal
// and log1p are predictive_math.h's (table exp, ~2 ulp; a NaN is put back where the clamp of the exp
// would lose it).  Chunks write partial totals; k_draw_totals sums them in chunk order, so the totals
// are bitwise independent of how many shards share a launch and of which GPU runs a shard.
#pragma once
#include "launchers.h"
#include "sweep_common.h"
#include "predictive_math.h"
#include <math.h>
#include <type_traits>
#include <utility>

namespace stk {

// k-steps per draw tile, and doubles per draw tile: the k-steps, 64 per-draw scalars, padded to a whole
// number of block-wide copies
__host__ __device__ constexpr int pred_kf(int d) { return (d + 3) / 4; }
__host__ __device__ constexpr int pred_slab(int kf) { return (kf * 64 + 64 + 255) / 256 * 256; }

// ---- chunk geometry: `units` row units, per_chunk of them to a chunk until the count saturates at gmax
__host__ __device__ constexpr int64_t draw_units(int64_t n, int rows) { return (n + rows - 1) / rows; }
__host__ __device__ constexpr int draw_chunks(int64_t units, int per_chunk, int gmax) {
  const int64_t g = (units + per_chunk - 1) / per_chunk;
  return (int)(g < 1 ? 1 : (g > gmax ? gmax : g));
}
struct UnitRange { int64_t first, last; };
__host__ __device__ inline UnitRange draw_chunk_units(int64_t units, int chunk, int G) {
  return {units * chunk / G, units * (chunk + 1) / G};
}

struct PredArgs {
  const ShardDev* shards;
  const double* img;        // [ntile][slab] the draw image
  double* partial;          // [nsh][Gs][8] chunk-partial totals
  double* rows;             // nullptr, or [sum n][4] per-row values, shard-major
  const int64_t* rowoff;    // [nsh] first row of every shard of the launch in `rows`
  double* totals;           // [nsh][8]
  int family, shard0, Gs, S, ntile;
};

// y of the lane's rows row0 + lg + 4 i (0 past n); poisson WITH_LGAMMA: lgamma(y + 1) once per row (lane
// lr takes row row0 + lr) and handed round
template <int FAM, bool WITH_LGAMMA>
__device__ __forceinline__ void draw_row_y(const ShardDev& sh, int64_t row0, int lr, int lg, double (&yv)[4],
                                           double (&lgam)[4]) {
  constexpr bool POIS = FAM == STK_POISSON && WITH_LGAMMA;
  double lgr = 0.0;
  if constexpr (POIS) {
    const int64_t row = row0 + lr;
    lgr = lgamma((row < sh.n ? (double)sh.yi[row] : 0.0) + 1.0);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = row0 + lg + 4 * i;
    yv[i] = 0.0;
    if (row < sh.n) yv[i] = FAM == STK_LINREG ? sh.y[row] : (double)sh.yi[row];
    lgam[i] = POIS ? __shfl(lgr, lg + 4 * i) : 0.0;
  }
}

// 16 rows from `base`, contiguous in HBM, into an LDS slot; thread i0 of `stride`.  Zero past lim.
__device__ __forceinline__ void draw_stage_rows(double* slot, gptr_t<double> xg, int64_t base, int64_t lim, int d, int i0,
                                                int stride) {
  for (int i = i0; i < 16 * d; i += stride) slot[i] = base + i < lim ? __builtin_nontemporal_load(xg + base + i) : 0.0;
}
// the slot's [16][d] rows as the lane's A operands: row lr, columns 4 s + lg
template <int KF>
__device__ __forceinline__ void draw_load_a(const double* slot, int d, int lr, int lg, double (&a)[KF]) {
#pragma unroll
  for (int s = 0; s < KF; ++s) {
    const int col = 4 * s + lg;
    a[s] = col < d ? slot[lr * d + col] : 0.0;
  }
}

// eta of rows lg + 4 i at draw lr, on two alternating accumulators; B: a slab in LDS.  (k_loo reads its
// slabs from global memory and has this loop, without the fence, written out: KEPT in loo.hip says why
// it also has copies of draw_row_y, draw_stage_rows, draw_load_a and the chunk count.  A change to one
// of those here belongs there too.)
template <int KF>
__device__ __forceinline__ dbl4 draw_eta(const double (&a)[KF], const double* B, double alpha, int lane) {
  dbl4 e0 = dbl4{alpha, alpha, alpha, alpha}, e1 = dbl4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < KF; ++s) {
    if (s & 1) e1 = mfma_f64(a[s], B[s * 64 + lane], e1);
    else e0 = mfma_f64(a[s], B[s * 64 + lane], e0);
    if ((s & 7) == 7) __builtin_amdgcn_sched_barrier(0);   // B reads at most 8 k-steps ahead: registers
  }
  return e0 + e1;
}

// ll of one (row, draw) and g, the mean of y there
template <int FAM>
__device__ __forceinline__ double draw_ll(double eta, double y, double lgam, double u, double e2u, const double* tab,
                                          double& g) {
  static_assert(FAM == STK_LINREG || FAM == STK_LOGREG || FAM == STK_POISSON, "draw_ll: unknown family");
  if constexpr (FAM == STK_LOGREG) {
    const double z = y != 0.0 ? eta : -eta;
    const double e = pd_exp(-fabs(eta), tab);
    const double r1 = pd_rcp(1.0 + e);
    const double lt = (z < 0.0 ? z : 0.0) - pd_log1p01(e);
    g = eta >= 0.0 ? r1 : e * r1;
    g = eta != eta ? eta : g;
    return eta != eta ? eta : lt;                    // pd_exp turns a NaN into 0: put it back
  } else if constexpr (FAM == STK_LINREG) {
    const double r = y - eta;
    g = eta;
    return -0.91893853320467274178 - u - 0.5 * (r * r) * e2u;
  } else {
    g = pd_exp(eta, tab);
    g = eta != eta ? eta : g;
    return y * eta - g - lgam;
  }
}

// The two-slot ring of draw-tile slabs a block of W waves shares: slab 0 straight in, then slab t + 1
// into registers while tile t's element work runs and into the other slot after it.  The caller's
// barrier follows fill_first and every commit.
template <int KF, int W>
struct SlabRing {
  static constexpr int SLAB = pred_slab(KF), NPF = SLAB / (64 * W);
  double* const ring;       // [2][SLAB]
  const gptr_t<double> img;
  const int tid;
  double pf[NPF];
  __device__ __forceinline__ const double* slab(int t) const { return ring + (t & 1) * SLAB; }
  __device__ __forceinline__ void fill_first() {
#pragma unroll
    for (int j = 0; j < NPF; ++j) {
      const int k = tid + 64 * W * j;
      ring[k] = img[k];
    }
  }
  __device__ __forceinline__ void prefetch(int t) {
#pragma unroll
    for (int j = 0; j < NPF; ++j) {
      const int k = tid + 64 * W * j;
      pf[j] = img[(size_t)t * SLAB + k];
    }
  }
  __device__ __forceinline__ void commit(int t) {
    double* Bn = ring + (t & 1) * SLAB;
#pragma unroll
    for (int j = 0; j < NPF; ++j) {
      const int k = tid + 64 * W * j;
      Bn[k] = pf[j];
    }
  }
};

// totals[s][1 + k] = the chunk partials of shard s summed in chunk order, k < LIVE; [0] = n, the rest 0
template <int (*CHUNKS)(int64_t), int LIVE>
__global__ __launch_bounds__(64) void k_draw_totals(PredArgs A, int nsh) {
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= nsh * 8) return;
  const int si = idx >> 3, k = idx & 7;
  const ShardDev sh = A.shards[A.shard0 + si];
  double v = 0.0;
  if (k == 0) {
    v = (double)sh.n;
  } else if (k <= LIVE) {
    const int G = CHUNKS(sh.n);
    const double* src = A.partial + (size_t)si * A.Gs * 8 + (k - 1);
    v = src[0];
    for (int c = 1; c < G; ++c) v += src[(size_t)c * 8];
  }
  A.totals[idx] = v;
}
template <int (*CHUNKS)(int64_t), int LIVE>
inline hipError_t launch_draw_totals(const PredArgs& A, int nsh, hipStream_t st) {
  hipLaunchKernelGGL((k_draw_totals<CHUNKS, LIVE>), dim3((nsh * 8 + 63) / 64), dim3(64), 0, st, A, nsh);
  return hipGetLastError();
}

// f(integral_constant FAM, integral_constant KF) for a regression family at 1 <= d <= 128 covariates
template <int FAM, class F, int... K>
hipError_t draw_dispatch_kf(int kf, F& f, std::integer_sequence<int, K...>) {
  hipError_t e = hipErrorInvalidValue;
  (void)((kf == K + 1 && ((e = f(std::integral_constant<int, FAM>{}, std::integral_constant<int, K + 1>{})), true)) || ...);
  return e;
}
template <class F>
hipError_t draw_dispatch(int family, int d, F f) {
  const std::make_integer_sequence<int, 32> kfs{};
  if (family == STK_LOGREG) return draw_dispatch_kf<STK_LOGREG>(pred_kf(d), f, kfs);
  if (family == STK_LINREG) return draw_dispatch_kf<STK_LINREG>(pred_kf(d), f, kfs);
  if (family == STK_POISSON) return draw_dispatch_kf<STK_POISSON>(pred_kf(d), f, kfs);
  return hipErrorInvalidValue;
}

}  // namespace stk
