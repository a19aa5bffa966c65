// The per-draw log-density sweep (regression families, 1 <= d <= 128): for every one of S draws, the
// log density of a shard at that draw -- the reduction of the sampler's sweeps (over rows, for each
// draw), at the width of the log-predictive sweep (any S, X read once for all of them) and without the
// backward pass the sweeps pay for a gradient.  It is what importance weights of a proposal are made of
// (the definitions are in include/stark_hip.h).  The second half of the file is
// the proposal itself: k_laplace_draws.
//
//   eta_is = alpha_s + x_i . beta_s           draw_forward.h's forward pass, for S draws
//   logistic  t = (2 y_i - 1) eta, e = exp(-|t|):  sum_i ll = sum (t - |t|) / 2 - log prod (1 + e)
//   poisson   sum_i ll = sum y_i eta - exp(eta)                                  (propto: no lgamma)
//   linear    the sweep carries sum (y_i - eta)^2; the reduce finishes -e^{-2u} sum / 2 - n u
//   lp_s = sum_i ll + prior + Jacobian, the terms of k_sweep_reduce (sweep.hip)
//
// k_logdens: k_predictive's launch shape (4 waves per block, two blocks per CU, chunks of whole 64-row
// groups, the slab ring) with the element work reduced the other way: the lane's four elements are summed
// (logistic: the four 1 + e multiplied and ONE log taken, the sweeps' running product cut at the tile --
// so not draw_ll, which takes a log1p per element), then the four lane groups in a fixed order: one
// number per (wave, draw).  The four waves' numbers meet in a small double-buffered LDS array; wave 0
// adds them in wave order to the chunk's running sum of that draw, which lives in the chunk's row of
// the partial buffer (read, add, write by the same lane every time: program order; the first group of
// a chunk writes without reading, so the buffer needs no zeroing).  A chunk's working set is S doubles:
// it stays in L2.
// Rows past n are masked out by select, never by a product, so a NaN draw stays NaN and a finite draw is
// never touched by a padding row.  Draw s is column s & 15 of tile s >> 4; an MFMA output column depends
// on its own B column only, every sum above runs in an order fixed by (n, d), and k_logdens_reduce adds
// the chunks in chunk order: lp_s depends on draw s and the shard alone, bit for bit -- not on S, on
// the position in q, on its companions or on how many shards share the launch.
#include "draw_forward.h"
#include <algorithm>

namespace stk {

constexpr int LD_R = 16;          // rows per wave tile = MFMA M
constexpr int LD_W = 4;           // waves per block
constexpr int LD_GPC = 4;         // 64-row groups per chunk before the chunk count saturates
constexpr int LD_GMAX = 256;      // chunks per shard at most
constexpr int LD_RED = 2 * LD_W * 16;   // the waves' per-draw sums of two tiles

__host__ __device__ inline int logdens_chunks(int64_t n) { return draw_chunks(draw_units(n, LD_R * LD_W), LD_GPC, LD_GMAX); }
// the exp table, the waves' sums, then ONE area that holds the four waves' rows while a group starts and
// the slab ring after
__host__ __device__ constexpr size_t logdens_lds_doubles(int d) {
  const size_t ring = (size_t)2 * pred_slab(pred_kf(d)), rows = (size_t)LD_W * LD_R * d;
  return EX_TAB + LD_RED + (ring > rows ? ring : rows);
}

struct LogdensArgs {
  const ShardDev* shards;
  const double* img;        // [ntile][slab] the draw image (k_predictive_prep)
  const double* q;          // [S][D] the draws (the reduce: prior and Jacobian)
  double* partial;          // [nsh][Gs][16 ntile] chunk-partial sums per draw
  double* lp;               // [nsh][S]
  int family, shard0, Gs, S, ntile, D;
};

template <int FAM, int KF>
__global__ __launch_bounds__(64 * LD_W, 2) void k_logdens(LogdensArgs A) {
  const int si = blockIdx.y, chunk = blockIdx.x;
  const ShardDev sh = A.shards[A.shard0 + si];
  const int G = logdens_chunks(sh.n);
  if (chunk >= G) return;                            // block-uniform
  const int d = sh.d;
  constexpr bool LIN = FAM == STK_LINREG, LOGI = FAM == STK_LOGREG, POIS = FAM == STK_POISSON;
  static_assert(LIN || LOGI || POIS, "k_logdens: unknown family");
  const int tid = threadIdx.x, lane = tid & 63, w = uniform_int(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4;

  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* const tab = lds;                           // [EX_TAB] 2^(j/1024)
  double* const red = lds + EX_TAB;                  // [2][LD_W][16] the waves' sums of a tile
  double* const ring = red + LD_RED;                 // [2][SLAB] draw-tile slabs
  double* const xs = ring + (size_t)w * LD_R * d;    // [16][d] the wave's rows, before the ring is filled
  if constexpr (!LIN) exp_table_init(tab);

  const UnitRange groups = draw_chunk_units(draw_units(sh.n, LD_R * LD_W), chunk, G);
  const gptr_t<double> xg = gp(sh.x);
  SlabRing<KF, LD_W> slabs{ring, gp(A.img), tid};
  const int64_t lim = sh.n * d;
  double* const acc = A.partial + ((size_t)si * A.Gs + chunk) * ((size_t)16 * A.ntile);

  // the four waves' sums of tile t, in wave order, onto the chunk's running sum (wave 0, lanes 0..15)
  auto flush = [&](int t, bool first) {
    if (w == 0 && lane < 16) {
      const double* r = red + (t & 1) * (LD_W * 16) + lane;
      const double v = ((r[0] + r[16]) + r[32]) + r[48];
      double* p = acc + (size_t)16 * t + lane;
      *p = first ? v : *p + v;
    }
  };

  for (int64_t grp = groups.first; grp < groups.last; ++grp) {
    const int64_t row0 = grp * (LD_R * LD_W) + w * LD_R;
    const bool first = grp == groups.first;
    double yv[4], lgam[4];                           // no lgamma here: propto
    bool ok[4];
    draw_row_y<FAM, false>(sh, row0, lr, lg, yv, lgam);
#pragma unroll
    for (int i = 0; i < 4; ++i) ok[i] = row0 + lg + 4 * i < sh.n;
    // ---- the wave's 16 rows into the A registers
    draw_stage_rows(xs, xg, row0 * d, lim, d, lane, 64);
    __syncthreads();
    double a[KF];
    draw_load_a<KF>(xs, d, lr, lg, a);
    __syncthreads();                                 // every wave has its rows: the area becomes the ring
    slabs.fill_first();
    __syncthreads();

#pragma nounroll                                      // one copy of the body
    for (int t = 0; t < A.ntile; ++t) {
      const double* B = slabs.slab(t);
      const dbl4 eta4 = draw_eta<KF>(a, B, B[KF * 64 + lr], lane);
      __builtin_amdgcn_sched_barrier(0);
      // the next slab, into registers while the element work runs (the B operands' registers are free now)
      if (t + 1 < A.ntile) slabs.prefetch(t + 1);
      if (t > 0) flush(t - 1, first);                // the barrier that ended tile t - 1 published its sums
      double v;
      if constexpr (LOGI) {
        double lm = 0.0, pr = 1.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double eta = eta4[i];
          const double z = yv[i] != 0.0 ? eta : -eta;
          const double e = pd_exp(-fabs(eta), tab);   // a NaN eta gives 0 here and stays NaN in lm
          lm += ok[i] ? z - fabs(z) : 0.0;
          pr *= ok[i] ? 1.0 + e : 1.0;
        }
        v = 0.5 * lm - log(pr);                      // pr in [1, 16]: four roundings, 4 eps of log
      } else if constexpr (POIS) {
        v = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double eta = eta4[i];
          double mu = pd_exp(eta, tab);
          mu = eta != eta ? eta : mu;                // pd_exp turns a NaN into 0: put it back
          const double term = fma(yv[i], eta, -mu);
          v += ok[i] ? term : 0.0;
        }
      } else {
        v = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double r = yv[i] - eta4[i];
          const double term = r * r;
          v += ok[i] ? term : 0.0;
        }
      }
      // the four lane groups of draw lr, in a fixed order; lanes of group 0 hand the wave's sum over
      const double v1 = __shfl(v, lr + 16), v2 = __shfl(v, lr + 32), v3 = __shfl(v, lr + 48);
      if (lg == 0) red[(t & 1) * (LD_W * 16) + w * 16 + lr] = ((v + v1) + v2) + v3;
      if (t + 1 < A.ntile) slabs.commit(t + 1);
      __syncthreads();
    }
    flush(A.ntile - 1, first);                       // before the next group's barriers: its slot is reused after them
  }
}

// lp[si][s] = the chunk partials of draw s summed in chunk order, then the family's closing terms, the
// normal(0, s) priors and the Jacobian of sigma = e^u, each once (k_sweep_reduce's formulas)
__global__ __launch_bounds__(256) void k_logdens_reduce(LogdensArgs A) {
  const int s = blockIdx.x * 256 + threadIdx.x, si = blockIdx.y;
  if (s >= A.S) return;
  const ShardDev sh = A.shards[A.shard0 + si];
  const int G = logdens_chunks(sh.n), d = sh.d;
  const size_t Sp = (size_t)16 * A.ntile;
  const double* src = A.partial + (size_t)si * A.Gs * Sp + s;
  double t = src[0];
  for (int c = 1; c < G; ++c) t += src[(size_t)c * Sp];
  const double* qc = A.q + (size_t)s * A.D;
  double prior_lp = 0.0;
  if (sh.pa != 0.0 || sh.pb != 0.0) {
    double sb = 0.0;
    for (int j = 1; j <= d; ++j) sb = fma(qc[j], qc[j], sb);
    prior_lp = -0.5 * (sh.pa * qc[0] * qc[0] + sh.pb * sb);
  }
  double lp;
  if (A.family == STK_LINREG) {
    const double u = qc[d + 1], N = (double)sh.n;
    lp = -0.5 * (t * exp(-2.0 * u)) - N * u + u + prior_lp;
  } else {
    lp = t + prior_lp;
  }
  A.lp[(size_t)si * A.S + s] = lp;
}

template <int FAM, int KF>
static hipError_t go_logdens(const LogdensArgs& A, int d, int nsh, hipStream_t st) {
  const size_t lds = logdens_lds_doubles(d) * sizeof(double);
  auto kern = k_logdens<FAM, KF>;
  if (lds > 64 * 1024)
    if (const hipError_t e = allow_big_lds(reinterpret_cast<const void*>(kern))) return e;
  hipLaunchKernelGGL(kern, dim3(A.Gs, nsh), dim3(64 * LD_W), lds, st, A);
  return hipGetLastError();
}

// ---------------------------------------------------------------- the Laplace proposal
// theta_s = mode + F xi_s with xi_{s,j} = normal_at(seed, stream, s, 0, j, TAG_LAPLACE) (philox.h: the
// counter is {stream, s, j / 2, TAG}), and log_q[s] = -sum_j xi_{s,j}^2 / 2 in index order.  One block
// per draw: thread j makes xi_j, thread i forms row i of the product in index order (fma), thread 0 the
// sum of squares.  A draw is a function of (seed, stream, s) and the call's mode and factor only.
constexpr int LAP_DMAX = 130;
struct LaplaceArgs {
  const double* mode;       // [D]
  const double* factor;     // [D][D] row-major
  double* q;                // [S][D]
  double* log_q;            // [S]
  uint64_t seed;
  uint32_t stream;
  int D, S;
};

__global__ __launch_bounds__(192) void k_laplace_draws(LaplaceArgs A) {
  __shared__ double xi[LAP_DMAX];
  const int s = blockIdx.x, i = threadIdx.x;
  if (i < A.D) xi[i] = normal_at(A.seed, A.stream, (uint32_t)s, 0u, (uint32_t)i, TAG_LAPLACE);
  __syncthreads();
  if (i < A.D) {
    const double* f = A.factor + (size_t)i * A.D;
    double v = 0.0;
    for (int j = 0; j < A.D; ++j) v = fma(f[j], xi[j], v);
    A.q[(size_t)s * A.D + i] = A.mode[i] + v;
  }
  if (i == 0) {
    double v = 0.0;
    for (int j = 0; j < A.D; ++j) v = fma(xi[j], xi[j], v);
    A.log_q[s] = -0.5 * v;
  }
}

}  // namespace stk

using namespace stk;

bool stk_logdens_supported(int d) { return d >= 1 && d <= 128; }
int stk_logdens_chunks(int64_t n) { return logdens_chunks(n); }
int stk_logdens_rows_per_tile() { return LD_R; }
int stk_logdens_waves() { return LD_W; }
size_t stk_logdens_lds_bytes(int d) { return logdens_lds_doubles(d) * sizeof(double); }
// chunk-partial workspace of one shard: a row of 16 ceil(S / 16) sums per chunk
size_t stk_logdens_ws_bytes(int64_t n, int S) {
  return sizeof(double) * 16 * (size_t)stk_predictive_tiles(S) * (size_t)logdens_chunks(n);
}

// Shards [shard0, shard0 + nsh) against the image of q [S][D] -> lp [nsh][S]; partial holds nsh * Gs
// chunk rows of 16 ceil(S / 16) doubles, Gs >= every shard's chunk count.  One sweep launch and one
// reduce launch for all of them.
hipError_t stk_launch_logdens(int family, const ShardDev* shards, int shard0, int nsh, int d, int D, int Gs, int S,
                              const double* img, const double* q, double* partial, double* lp, hipStream_t st) {
  const LogdensArgs A{shards, img, q, partial, lp, family, shard0, Gs, S, stk_predictive_tiles(S), D};
  const hipError_t e = draw_dispatch(family, d, [&](auto fam, auto kf) {
    return go_logdens<decltype(fam)::value, decltype(kf)::value>(A, d, nsh, st);
  });
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_logdens_reduce, dim3((unsigned)((S + 255) / 256), nsh), dim3(256), 0, st, A);
  return hipGetLastError();
}

int stk_laplace_max_dim() { return LAP_DMAX; }

hipError_t stk_launch_laplace_draws(const double* mode, const double* factor, int D, int S, uint64_t seed,
                                    uint32_t stream, double* q, double* log_q, hipStream_t st) {
  const LaplaceArgs A{mode, factor, q, log_q, seed, stream, D, S};
  hipLaunchKernelGGL(k_laplace_draws, dim3((unsigned)S), dim3(192), 0, st, A);
  return hipGetLastError();
}
