// The PSIS-LOO sweep (regression families, 1 <= d <= 128, 1 <= S <= 1024): for every ROW of a shard,
// Pareto-smoothed importance-sampling leave-one-out over S posterior draws -- elpd_loo, the Pareto shape
// khat of the row's importance-ratio tail, lppd and p_loo (DESIGN.md sections 3 and 8; the definitions
// are in include/stark_hip.h, the per-row arithmetic in psis_math.h).  No reference counterpart.
//
// The n x S matrix of log ratios never reaches HBM: a workgroup owns one 16-row MFMA tile at a time and
// keeps the tile's [16][Sp] log ratios in LDS (Sp = S padded to a power of two, 128 KB at Sp = 1024).
//
//   forward   draw_forward.h's forward pass; ll is its draw_ll, the other pieces are written out here (KEPT,
//             below).  The tile's 16 rows go into EVERY wave's registers as the same A
//             operand.  The waves split the 16-draw tiles of the image (tile t to wave t mod W); a slab
//             is read by exactly one wave of the block, so its B operands come straight from global
//             memory (L2) into registers, 512 B per k-step, with no LDS ring.  The wave writes
//             lr = -ll to mat[row][draw].  A draw lane of the last tile past S and the columns up
//             to Sp hold -inf, which sorts to the front.  A non-finite ll sets the row's flag (1: -inf,
//             2: NaN, 4: +inf) and is stored as +inf (-inf for ll = +inf), so the sort never meets a NaN.
//   sort      A block is W = 4 waves (8 from Sp = 512).  Wave w takes the 16 / W rows from (16 / W) w and
//             sorts each ascending in LDS with a bitonic network, its rows interleaved in one stage
//             loop.  A row belongs to one wave, so stages are separated by a wavefront-scope fence (a
//             wave's LDS operations complete in order), not a workgroup barrier.
//   fit       Per row, psis_math.h's pieces with one lane per grid point (<= 39 live lanes; a lane loops
//             over the <= 96 exceedances, broadcast LDS reads in ascending order, so the inner loop has no
//             cross-lane reduction) and one lane per tail value; sums over grid points run serially in
//             index order in every lane.  The per-wave scratch lies where the row slot was.
//   reduce    The three logsumexps over the S sorted values: lane-strided, then fixed-order xor
//             butterflies over the 64 lanes.  ll is paired through the sort as -lr.
// LDS banks: a forward store is ds_write_b64 by 16-lane groups, each writing 16 consecutive doubles (32
// banks of 32): conflict-free at any row stride.  The sort and the sums touch one row per instruction,
// so the row stride is Sp with no padding; compare-exchange strides below 32 read two-way conflicted.
//
// A shard is cut into G chunks of whole 16-row tiles, G a function of n alone (and W of S alone).  A
// row's four values depend only on (x_i, y_i) and the draws.  A chunk's partial totals are summed in
// wave order, then row order.
#include "draw_forward.h"
#include "psis_math.h"
#include <algorithm>

namespace stk {

constexpr int LO_R = 16;          // rows per tile = MFMA M
constexpr int LO_WMAX = 8;        // waves per block: 8 from Sp = 512 (the matrix leaves room for one block per CU,
                                  // so a second wave per SIMD is what hides the sort's LDS latency), else 4
constexpr int LO_TPC = 2;         // tiles per chunk before the chunk count saturates
constexpr int LO_GMAX = 512;      // chunks per shard at most
constexpr int LO_SCR = PSIS_MMAX + 2 * 40;   // per-wave scratch doubles: exceedances, profile, theta * weight

// KEPT.  k_loo shares with draw_forward.h only what leaves every one of its instantiations the instructions
// it had before that header existed: draw_ll and draw_chunk_units.  With any of draw_chunks (below),
// draw_row_y, draw_stage_rows, draw_load_a or a PredArgs inside LooArgs, the compiler orders and places
// the same work differently, and the 4-wave kernel at S = 256 then ran 0.5 to 1 % slower in every run
// (8 shards x 1.25e7 rows, d = 100); with draw_eta the 8-wave linear kernels at KF 29, 31, 32 also spilled.
// So those pieces stand here as k_predictive had them; tools/codeobj_compare.py shows whether a change
// to either copy still leaves k_loo's text alone.
__host__ __device__ inline int loo_chunks(int64_t n) {   // draw_chunks(draw_units(n, LO_R), LO_TPC, LO_GMAX)
  const int64_t nt = (n + LO_R - 1) / LO_R, g = (nt + LO_TPC - 1) / LO_TPC;
  return (int)(g < 1 ? 1 : (g > LO_GMAX ? LO_GMAX : g));
}
__host__ __device__ inline int loo_sp(int S) {       // S padded to a power of two, at least one draw tile
  int p = 16;
  while (p < S) p <<= 1;
  return p;
}
__host__ __device__ inline int loo_waves(int S) { return loo_sp(S) >= 512 ? LO_WMAX : 4; }
// one area: the tile's rows during the forward, the waves' scratch after it
__host__ __device__ constexpr int loo_area(int d) { return LO_R * d > LO_WMAX * LO_SCR ? LO_R * d : LO_WMAX * LO_SCR; }
// exp table, the area, the matrix, 16 row flags
__host__ __device__ inline size_t loo_lds_doubles(int d, int S) {
  return (size_t)EX_TAB + loo_area(d) + (size_t)LO_R * loo_sp(S) + LO_R / 2;
}

// PredArgs's fields, then three more -- written out, not derived: a PredArgs base or member is padded to 72
// bytes and moves Sp, M and Mg in the kernel's argument segment, which is among what KEPT below is about
struct LooArgs {
  const ShardDev* shards;
  const double* img;        // [ntile][slab] the draw image
  double* partial;          // [nsh][Gs][8] chunk-partial totals
  double* rows;             // nullptr, or [sum n][4] (elpd_loo, khat, lppd, p_loo), shard-major
  const int64_t* rowoff;    // [nsh] first row of every shard of the launch in `rows`
  double* totals;           // [nsh][8]
  int family, shard0, Gs, S, ntile;
  int Sp, M, Mg;            // loo_sp(S), psis_tail_len(S), psis_grid(M)
};

// Orders a wave's own LDS writes before its later reads (lanes exchange data through LDS).
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_xor(v, o);
    v = u > v ? u : v;
  }
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

// logsumexp_s ll_s - log S from the sorted lr = -ll of a row whose ll may hold -inf (lr = +inf: adds 0)
__device__ __forceinline__ double loo_lppd(const double* v, int S, const double* tab, int lane, double logS) {
  constexpr double INF = __builtin_huge_val();
  const double m3 = -v[0];
  double s3 = 0.0;
  for (int k = lane; k < S; k += 64) s3 += pd_exp(-v[k] - m3, tab);
  s3 = wave_sum(s3);
  return m3 > -INF ? m3 + log(s3) - logS : -INF;
}

// One finite row: v [S] sorted ascending, scr the wave's scratch.  Every lane returns the same values.
__device__ __forceinline__ void loo_row(const double* v, const LooArgs& A, const double* tab, double* scr, int lane,
                                        double logS, double& elpd, double& khat, double& lppd) {
  constexpr double INF = __builtin_huge_val();
  const int S = A.S, M = A.M, Mg = A.Mg;
  double* x = scr;
  double* l = scr + PSIS_MMAX;
  double* tw = l + 40;
  const double mx = v[S - 1];
  khat = INF;
  bool smoothed = false;
  if (M >= 5 && (v[S - 1] - mx) - (v[S - M] - mx) > 0.0) {       // wave-uniform: LDS values
    const double ecut = exp(v[S - M - 1] - mx);
    for (int i = lane; i < M; i += 64) x[i] = exp(v[S - M + i] - mx) - ecut;
    wave_sync();
    const double xN = x[M - 1], xstar = x[psis_xstar_index(M) - 1];
    const int j = lane < Mg ? lane + 1 : Mg;                     // idle lanes repeat the last grid point
    const double th = psis_theta(j, Mg, xN, xstar);
    const double lj = psis_profile(th, psis_kbar(th, x, M), M);
    if (lane < Mg) l[lane] = lj;
    wave_sync();
    const double wj = psis_weight(l, Mg, j - 1, tab);
    if (lane < Mg) tw[lane] = th * wj;
    wave_sync();
    double that = 0.0;
    for (int i = 0; i < Mg; ++i) that += tw[i];
    const double k = psis_kbar(that, x, M), sigma = -k / that;
    khat = psis_khat(k, M);
    wave_sync();                                                 // every lane has read x
    if (khat - khat == 0.0) {
      smoothed = true;
      for (int i = lane; i < M; i += 64) x[i] = psis_smooth(i + 1, M, sigma, khat, ecut);
    }
    wave_sync();
  }
  double m1 = -INF, m2 = -INF;
  for (int k = lane; k < S; k += 64) {
    const double lw = psis_lw(v, k, S, M, smoothed, x), b = lw - v[k];
    m1 = lw > m1 ? lw : m1;
    m2 = b > m2 ? b : m2;
  }
  m1 = wave_max(m1);
  m2 = wave_max(m2);
  const double m3 = -v[0];
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int k = lane; k < S; k += 64) {
    const double lw = psis_lw(v, k, S, M, smoothed, x);
    s1 += pd_exp(lw - m1, tab);
    s2 += pd_exp((lw - v[k]) - m2, tab);
    s3 += pd_exp(-v[k] - m3, tab);
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  s3 = wave_sum(s3);
  elpd = (m2 + log(s2)) - (m1 + log(s1));
  lppd = m3 + log(s3) - logS;
  wave_sync();                                                   // the scratch is free for the next row
}

template <int FAM, int KF, int LO_W>
__global__ __launch_bounds__(64 * LO_W) void k_loo(LooArgs A) {
  constexpr int SLAB = pred_slab(KF), LO_RPW = LO_R / LO_W;   // rows a wave sorts and fits
  constexpr double INF = __builtin_huge_val(), NINF = -INF;
  const int si = blockIdx.y, chunk = blockIdx.x;
  const ShardDev sh = A.shards[A.shard0 + si];
  const int G = loo_chunks(sh.n);
  if (chunk >= G) return;                            // block-uniform
  const int d = sh.d, S = A.S, Sp = A.Sp;
  constexpr bool LIN = FAM == STK_LINREG, POIS = FAM == STK_POISSON;
  const int tid = threadIdx.x, lane = tid & 63, w = uniform_int(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4;

  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* const tab = lds;                           // [EX_TAB] 2^(j/1024)
  double* const area = lds + EX_TAB;                 // [16][d] the tile's rows | [LO_W][LO_SCR] scratch (loo_area)
  double* const mat = area + loo_area(d);            // [16][Sp] lr = -ll
  int* const flags = reinterpret_cast<int*>(mat + (size_t)LO_R * Sp);   // [16]
  exp_table_init(tab);

  const UnitRange tiles = draw_chunk_units(draw_units(sh.n, LO_R), chunk, G);
  const gptr_t<double> xg = gp(sh.x);
  const gptr_t<double> img = gp(A.img);
  const int64_t lim = sh.n * d;
  const double logS = log((double)S);
  const int padc = Sp - 16 * A.ntile;                // columns no draw tile writes
  double tot[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // sum lppd, p_loo, elpd, elpd^2, #k > 0.5, #k > 0.7, #non-finite

  for (int64_t tile = tiles.first; tile < tiles.last; ++tile) {
    const int64_t row0 = tile * LO_R;
    // draw_row_y<FAM, true> (KEPT): y of rows lg + 4 i; poisson: lgamma(y + 1) once per row and handed round
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
    // ---- draw_stage_rows and draw_load_a (KEPT): the tile's 16 rows into every wave's A registers
    const int64_t base = row0 * d;
    for (int i = tid; i < LO_R * d; i += 64 * LO_W) area[i] = base + i < lim ? __builtin_nontemporal_load(xg + base + i) : 0.0;
    if (tid < LO_R) flags[tid] = 0;
    for (int i = tid; i < LO_R * padc; i += 64 * LO_W) mat[(size_t)(i / padc) * Sp + 16 * A.ntile + i % padc] = NINF;
    __syncthreads();
    double a[KF];
#pragma unroll
    for (int s = 0; s < KF; ++s) {
      const int col = 4 * s + lg;
      a[s] = col < d ? area[lr * d + col] : 0.0;
    }

    // ---- forward: draw tile t to wave t mod W, B operands from global memory
#pragma nounroll
    for (int t = w; t < A.ntile; t += LO_W) {
      const gptr_t<double> B = img + (size_t)t * SLAB;
      const double alpha = B[KF * 64 + lr], u = B[KF * 64 + 16 + lr], e2u = B[KF * 64 + 32 + lr];
      const bool live = B[KF * 64 + 48 + lr] != 0.0;
      // draw_eta's loop (KEPT), without its (s & 7) fence and with B in global memory
      dbl4 e0 = dbl4{alpha, alpha, alpha, alpha}, e1 = dbl4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < KF; ++s) {
        if (s & 1) e1 = mfma_f64(a[s], B[s * 64 + lane], e1);
        else e0 = mfma_f64(a[s], B[s * 64 + lane], e0);
      }
      const dbl4 eta4 = e0 + e1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double g;                                    // not used here
        const double ll = draw_ll<FAM>(eta4[i], yv[i], lgam[i], u, e2u, tab, g);
        const int row = lg + 4 * i;
        double v = -ll;
        if (!live) {
          v = NINF;
        } else if (!(ll - ll == 0.0)) {              // -inf, NaN, +inf
          atomicOr(&flags[row], ll != ll ? 2 : (ll > 0.0 ? 4 : 1));
          v = ll > 0.0 ? NINF : INF;
        }
        mat[(size_t)row * Sp + 16 * t + lr] = v;
      }
    }
    __syncthreads();                                 // the matrix is whole; the slot becomes the scratch

    // ---- sort: the wave's LO_RPW rows, ascending, the padding first
    double* const mr = mat + (size_t)(LO_RPW * w) * Sp;
    for (int k = 2; k <= Sp; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int p = lane; p < (Sp >> 1); p += 64) {
          const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
          const bool up = (i & k) == 0;
#pragma unroll
          for (int q = 0; q < LO_RPW; ++q) {
            double* const r = mr + (size_t)q * Sp;
            const double x0 = r[i], x1 = r[i + j];
            const bool sw = up ? x1 < x0 : x0 < x1;
            r[i] = sw ? x1 : x0;
            r[i + j] = sw ? x0 : x1;
          }
        }
        wave_sync();
      }
    }

    // ---- fit and reduce, one row at a time
    double* const scr = area + w * LO_SCR;
    for (int q = 0; q < LO_RPW; ++q) {
      const int rl = LO_RPW * w + q;
      const int64_t row = row0 + rl;
      if (row >= sh.n) break;                        // wave-uniform
      const double* v = mat + (size_t)rl * Sp + (Sp - S);
      const int flag = flags[rl];
      double elpd, khat, lppd;
      if (flag == 0) {
        loo_row(v, A, tab, scr, lane, logS, elpd, khat, lppd);
      } else {
        const double nan = __builtin_nan("");
        elpd = khat = nan;
        lppd = (flag & 2) ? nan : ((flag & 4) ? INF : loo_lppd(v, S, tab, lane, logS));
      }
      const double ploo = lppd - elpd;
      tot[0] += lppd;
      tot[1] += ploo;
      tot[2] += elpd;
      tot[3] = fma(elpd, elpd, tot[3]);
      tot[4] += khat > 0.5 ? 1.0 : 0.0;
      tot[5] += khat > 0.7 ? 1.0 : 0.0;
      tot[6] += (elpd - elpd == 0.0 && lppd - lppd == 0.0 && ploo - ploo == 0.0 && khat == khat) ? 0.0 : 1.0;
      if (A.rows && lane < 4) {
        const double o = lane == 0 ? elpd : (lane == 1 ? khat : (lane == 2 ? lppd : ploo));
        A.rows[(A.rowoff[si] + row) * 4 + lane] = o;
      }
    }
    __syncthreads();                                 // every wave is done with the matrix and the scratch
  }

  // ---- block totals: every lane of a wave holds the wave's sums; wave order
  double* red = area;                                // [LO_W][8]
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 7; ++k) red[w * 8 + k] = tot[k];
  }
  __syncthreads();
  if (tid < 7) {
    double v = 0.0;
    for (int j = 0; j < LO_W; ++j) v += red[j * 8 + tid];
    A.partial[((size_t)si * A.Gs + chunk) * 8 + tid] = v;
  }
}

template <int FAM, int KF>
static hipError_t go_loo(const LooArgs& A, int d, int nsh, hipStream_t st) {
  const size_t lds = loo_lds_doubles(d, A.S) * sizeof(double);
  if (loo_waves(A.S) == LO_WMAX) {
    auto kern = k_loo<FAM, KF, LO_WMAX>;
    if (const hipError_t e = allow_big_lds(reinterpret_cast<const void*>(kern))) return e;
    hipLaunchKernelGGL(kern, dim3(A.Gs, nsh), dim3(64 * LO_WMAX), lds, st, A);
  } else {
    auto kern = k_loo<FAM, KF, 4>;
    if (lds > 64 * 1024)
      if (const hipError_t e = allow_big_lds(reinterpret_cast<const void*>(kern))) return e;
    hipLaunchKernelGGL(kern, dim3(A.Gs, nsh), dim3(64 * 4), lds, st, A);
  }
  return hipGetLastError();
}

}  // namespace stk

using namespace stk;

bool stk_loo_supported(int d) { return d >= 1 && d <= 128; }
int stk_loo_max_draws() { return PSIS_SMAX; }
int stk_loo_chunks(int64_t n) { return loo_chunks(n); }
int stk_loo_rows_per_tile() { return LO_R; }
int stk_loo_waves(int S) { return loo_waves(S); }
size_t stk_loo_lds_bytes(int d, int S) { return loo_lds_doubles(d, S) * sizeof(double); }
size_t stk_loo_ws_bytes(int64_t n) { return sizeof(double) * 8 * (size_t)loo_chunks(n); }

// Shards [shard0, shard0 + nsh) against the image -> totals [nsh][8] and, unless rows is null, the
// per-row values at rowoff[s] (device array of nsh offsets); partial holds nsh * Gs chunks of 8
// doubles, Gs >= every shard's chunk count.  One sweep launch and one reduce launch for all of them.
hipError_t stk_launch_loo(int family, const ShardDev* shards, int shard0, int nsh, int d, int Gs, int S,
                          const double* img, double* partial, double* rows, const int64_t* rowoff, double* totals,
                          hipStream_t st) {
  if (S < 1 || S > PSIS_SMAX || !stk_loo_supported(d)) return hipErrorInvalidValue;
  const int M = psis_tail_len(S);
  const PredArgs P{shards, img, partial, rows, rowoff, totals, family, shard0, Gs, S, stk_predictive_tiles(S)};
  const LooArgs A{P.shards, P.img, P.partial, P.rows, P.rowoff, P.totals, P.family, P.shard0, P.Gs, P.S, P.ntile,
                  loo_sp(S), M, psis_grid(M)};
  if (loo_lds_doubles(d, S) * sizeof(double) > BIG_LDS_BYTES) return hipErrorInvalidValue;
  const hipError_t e = draw_dispatch(family, d, [&](auto fam, auto kf) {
    return go_loo<decltype(fam)::value, decltype(kf)::value>(A, d, nsh, st);
  });
  return e != hipSuccess ? e : launch_draw_totals<loo_chunks, 7>(P, nsh, st);
}
