// The posterior predictive replicate sweep (regression families, 1 <= d <= 128, any S): for every row i of a
// shard and every draw s, a replicate y_rep_is drawn in the kernel from the family's sampling distribution at
// eta_is, reduced both ways -- over rows for each draw (the statistics of a replicated data set and the Pearson
// discrepancies of replicate and data) and, optionally, over draws for each row.  It is the generated
// quantities block of a Stan model, for the fixed families (the definitions are in
// include/stark_hip.h, the generator in yrep_math.h).
//
// k_yrep: k_logdens's launch shape (4 waves per block, two blocks per CU, chunks of whole 64-row groups that
// depend on n only, the wave's 16 rows as the A operand in registers, the slab ring) and draw_forward.h's
// forward pass.  Per draw tile a lane holds eta of rows lg + 4 i at draw lr; for each of the four it forms the
// family's mean and variance, one Philox call keyed by (row in shard, global draw index, stream) and the
// replicate, and sums seven numbers over its four rows: sum y_rep, sum y_rep^2, max, min, the two counts (zeros,
// and NaNs times 1024: one number), D(y_rep, theta), D(y, theta).  The four lane groups are joined in a fixed
// order, the four waves meet in a double-buffered LDS array, and threads 0 .. 127 (slot, draw column) join them
// in wave order onto the chunk's running values in the partial buffer (read, combine, write by the same thread
// every time; the first group of a chunk writes without reading).  k_yrep_reduce joins the chunks in chunk
// order.  Extrema skip a NaN replicate on the way and are made NaN at the end from the NaN count, so they need
// no NaN-propagating maximum.  Rows past n are masked by select, never by a product.
// Where the four elements of a lane are interleaved the generators spill (Poisson's inlines an lgamma and a
// 64-attempt loop), so every instantiation but the stats-only logistic one runs them in a loop (SERIAL below).
// ROWS: the per-row state (four numbers for each of the lane's four rows, streamed over the live draws and
// joined by a fixed-order xor butterfly over the 16 draw lanes, as k_predictive does it) is a second
// instantiation, so the stats-only sweep does not carry its registers.
// Draw s is column s & 15 of tile s >> 4 of the image, and its Philox counter carries draw0 + s; an element
// depends on (seed, stream, row, draw0 + s, eta, u) alone, every sum runs in an order fixed by n: no output
// depends on S, on the draw's position in q, on its companions or on how many shards share the launch.
#include "draw_forward.h"
#include "yrep_math.h"
#include <algorithm>

namespace stk {

constexpr int PP_R = 16;          // rows per wave tile = MFMA M
constexpr int PP_W = 4;           // waves per block
constexpr int PP_GPC = 4;         // 64-row groups per chunk before the chunk count saturates
constexpr int PP_GMAX = 256;      // chunks per shard at most
constexpr int PP_NS = 8;          // statistics per draw
constexpr int PP_LS = 7;          // numbers per (wave, draw) in LDS: the two counts share one
constexpr int PP_RED = 2 * PP_W * PP_LS * 16;
constexpr double PP_PACK = 1024.0;   // zeros + PP_PACK * NaNs: at most 16 rows per (wave, draw)

__host__ __device__ inline int ppc_chunks(int64_t n) { return draw_chunks(draw_units(n, PP_R * PP_W), PP_GPC, PP_GMAX); }
// the exp table, the waves' numbers, then ONE area that holds the four waves' rows while a group starts and
// the slab ring after: 80,896 bytes at d = 128, two blocks in a CU's 160 KiB
__host__ __device__ constexpr size_t ppc_lds_doubles(int d) {
  const size_t ring = (size_t)2 * pred_slab(pred_kf(d)), rows = (size_t)PP_W * PP_R * d;
  return EX_TAB + PP_RED + (ring > rows ? ring : rows);
}

struct PpcArgs {
  const ShardDev* shards;
  const double* img;        // [ntile][slab] the draw image (k_predictive_prep)
  double* partial;          // [nsh][Gs][ntile][8][16] chunk-partial statistics per draw
  double* opart;            // [nsh][Gs][8] chunk-partial statistics of the observed y
  double* stats;            // [nsh][S][8]
  double* obs;              // nullptr, or [nsh][8]
  double* rows;             // nullptr, or [sum n][4], shard-major
  double* yrep;             // nullptr, or [sum n][S], shard-major
  const int64_t* rowoff;    // [nsh] first row of every shard of the launch in rows / yrep
  const int32_t* streams;   // [nsh] RNG stream of every shard of the launch
  uint64_t seed;
  int family, shard0, Gs, S, ntile, draw0;
};

// slot k of two partial results joined: sums add, [2] is a maximum, [3] a minimum
__device__ __forceinline__ double ppc_join(int k, double a, double b) {
  return k == 2 ? (b > a ? b : a) : (k == 3 ? (b < a ? b : a) : a + b);
}

template <int FAM, int KF, bool ROWS>
__global__ __launch_bounds__(64 * PP_W, 2) void k_yrep(PpcArgs A) {
  constexpr double INF = __builtin_huge_val();
  const int si = blockIdx.y, chunk = blockIdx.x;
  const ShardDev sh = A.shards[A.shard0 + si];
  const int G = ppc_chunks(sh.n);
  if (chunk >= G) return;                            // block-uniform
  const int d = sh.d;
  constexpr bool LIN = FAM == STK_LINREG, LOGI = FAM == STK_LOGREG, POIS = FAM == STK_POISSON;
  static_assert(LIN || LOGI || POIS, "k_yrep: unknown family");
  // The lane's four elements one after the other in a loop that is not unrolled, everywhere but in the stats-only
  // logistic sweep (which has no spill unrolled, at any d): the compiler then holds one generator's registers,
  // not four interleaved ones.  The order of every sum is the same either way.
  constexpr bool SERIAL = !(LOGI && !ROWS);
  const int tid = threadIdx.x, lane = tid & 63, w = uniform_int(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4;

  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* const tab = lds;                           // [EX_TAB] 2^(j/1024)
  double* const red = lds + EX_TAB;                  // [2][PP_W][PP_LS][16] the waves' numbers of a tile
  double* const ring = red + PP_RED;                 // [2][SLAB] draw-tile slabs
  double* const xs = ring + (size_t)w * PP_R * d;    // [16][d] the wave's rows, before the ring is filled
  if constexpr (!LIN) exp_table_init(tab);

  const UnitRange groups = draw_chunk_units(draw_units(sh.n, PP_R * PP_W), chunk, G);
  const gptr_t<double> xg = gp(sh.x);
  SlabRing<KF, PP_W> slabs{ring, gp(A.img), tid};
  const int64_t lim = sh.n * d;
  const uint32_t stream = (uint32_t)A.streams[si];
  const int64_t out0 = A.rowoff[si];
  double* const acc = A.partial + ((size_t)si * A.Gs + chunk) * ((size_t)(PP_NS * 16) * A.ntile);

  // the four waves' numbers of tile t, in wave order, onto the chunk's running values: thread (slot k, column c)
  auto flush = [&](int t, bool first) {
    if (tid < PP_NS * 16) {
      const int k = tid >> 4, c = tid & 15;
      const bool cnt = k == 4 || k == 7;
      const double* r = red + (t & 1) * (PP_W * PP_LS * 16) + (k == 7 ? 4 : k) * 16 + c;
      double v = 0.0;
#pragma unroll
      for (int ww = 0; ww < PP_W; ++ww) {
        double x = r[ww * (PP_LS * 16)];
        if (cnt) {
          const double hi = floor(x * (1.0 / PP_PACK));
          x = k == 7 ? hi : x - PP_PACK * hi;
        }
        v = ww == 0 ? x : ppc_join(k, v, x);
      }
      double* p = acc + (size_t)(PP_NS * 16) * t + tid;
      *p = first ? v : ppc_join(k, *p, v);
    }
  };

  for (int64_t grp = groups.first; grp < groups.last; ++grp) {
    const int64_t row0 = grp * (PP_R * PP_W) + w * PP_R;
    const bool first = grp == groups.first;
    double yv[4], lgam[4];                           // no lgamma of y here
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

    double rlt[4], req[4], rs1[4], rs2[4];           // per row: #{y_rep < y}, #{y_rep = y}, sum y_rep, sum y_rep^2
#pragma unroll
    for (int i = 0; i < 4; ++i) rlt[i] = req[i] = rs1[i] = rs2[i] = 0.0;

#pragma nounroll                                      // one copy of the body
    for (int t = 0; t < A.ntile; ++t) {
      const double* B = slabs.slab(t);
      const double alpha = B[KF * 64 + lr], u = B[KF * 64 + 16 + lr], e2u = B[KF * 64 + 32 + lr];
      const bool live = B[KF * 64 + 48 + lr] != 0.0;
      const dbl4 eta4 = draw_eta<KF>(a, B, alpha, lane);
      __builtin_amdgcn_sched_barrier(0);
      // the next slab, into registers while the element work runs (the B operands' registers are free now)
      if (t + 1 < A.ntile) slabs.prefetch(t + 1);
      if (t > 0) flush(t - 1, first);                // the barrier that ended tile t - 1 published its numbers
      const uint32_t s = (uint32_t)(A.draw0 + 16 * t + lr);
      const double sigma = LIN ? exp(u) : 0.0;
      double v0 = 0.0, v1 = 0.0, vmax = -INF, vmin = INF, vc = 0.0, v5 = 0.0, v6 = 0.0;
      // one (row, draw): the family's mean and variance, the replicate, the lane's sums
      auto element = [&](int i, double eta, double yo, bool oki) {
        const int64_t row = row0 + lg + 4 * i;
        const YrepKey key = yrep_key(A.seed, stream, row, s);
        double U, V, y, trep, tobs;
        yrep_uv(key, 0u, U, V);
        if constexpr (LOGI) {
          double g, omg, var;
          yrep_logistic_mean(eta, tab, g, omg, var);
          y = yrep_logistic(U, g, nullptr);
          const double rr = y != 0.0 ? omg : -g, ro = yo != 0.0 ? omg : -g, iv = 1.0 / var;
          trep = var == 0.0 ? (rr == 0.0 ? 0.0 : INF) : rr * rr * iv;
          tobs = var == 0.0 ? (ro == 0.0 ? 0.0 : INF) : ro * ro * iv;
        } else if constexpr (POIS) {
          const double mu = yrep_poisson_mean(eta, tab);
          y = yrep_poisson(key, U, V, mu, tab, nullptr);
          const double rr = y - mu, ro = yo - mu, iv = 1.0 / mu;
          trep = mu == 0.0 ? (rr == 0.0 ? 0.0 : INF) : rr * rr * iv;
          tobs = mu == 0.0 ? (ro == 0.0 ? 0.0 : INF) : ro * ro * iv;
        } else {
          y = yrep_linear(U, V, eta, sigma);
          const double rr = y - eta, ro = yo - eta;
          trep = rr * rr * e2u;
          tobs = ro * ro * e2u;
        }
        const bool bad = y != y;
        trep = bad ? y : trep;
        v0 += oki ? y : 0.0;
        v1 += oki ? y * y : 0.0;
        vmax = oki && y > vmax ? y : vmax;           // a NaN is skipped here: the reduce puts it back
        vmin = oki && y < vmin ? y : vmin;
        vc += oki ? (y == 0.0 ? 1.0 : 0.0) + (bad ? PP_PACK : 0.0) : 0.0;
        v5 += oki ? trep : 0.0;
        v6 += oki ? tobs : 0.0;
        if (A.yrep && oki && live) A.yrep[(size_t)(out0 + row) * A.S + (16 * t + lr)] = y;
        if constexpr (ROWS) {
          const double lt = live && y < yo ? 1.0 : 0.0, eq = live && y == yo ? 1.0 : 0.0;
          const double a1 = live ? y : 0.0, a2 = live ? y * y : 0.0;
#pragma unroll
          for (int k = 0; k < 4; ++k) {                // a select of the addend: a NaN reaches its own row only
            rlt[k] += k == i ? lt : 0.0;
            req[k] += k == i ? eq : 0.0;
            rs1[k] += k == i ? a1 : 0.0;
            rs2[k] += k == i ? a2 : 0.0;
          }
        }
      };
      if constexpr (SERIAL) {
#pragma nounroll                                      // one copy of the generator, one element's registers
        for (int i = 0; i < 4; ++i)
          element(i, i == 0 ? eta4[0] : (i == 1 ? eta4[1] : (i == 2 ? eta4[2] : eta4[3])),
                  i == 0 ? yv[0] : (i == 1 ? yv[1] : (i == 2 ? yv[2] : yv[3])),
                  i == 0 ? ok[0] : (i == 1 ? ok[1] : (i == 2 ? ok[2] : ok[3])));
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) element(i, eta4[i], yv[i], ok[i]);
      }
      // the four lane groups of draw lr, in a fixed order; lanes of group 0 hand the wave's numbers over
      double* const rw = red + (t & 1) * (PP_W * PP_LS * 16) + w * (PP_LS * 16) + lr;
      const double val[PP_LS] = {v0, v1, vmax, vmin, vc, v5, v6};
#pragma unroll
      for (int k = 0; k < PP_LS; ++k) {
        const double x1 = __shfl(val[k], lr + 16), x2 = __shfl(val[k], lr + 32), x3 = __shfl(val[k], lr + 48);
        const double x = ppc_join(k, ppc_join(k, ppc_join(k, val[k], x1), x2), x3);
        if (lg == 0) rw[k * 16] = x;
      }
      if (t + 1 < A.ntile) slabs.commit(t + 1);
      __syncthreads();
    }
    flush(A.ntile - 1, first);                       // before the next group's barriers: its slot is reused after them

    if constexpr (ROWS) {
      // ---- the 16 draw lanes of every row, in a fixed order
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double c0 = rlt[i], c1 = req[i], c2 = rs1[i], c3 = rs2[i];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          c0 += __shfl_xor(c0, o);
          c1 += __shfl_xor(c1, o);
          c2 += __shfl_xor(c2, o);
          c3 += __shfl_xor(c3, o);
        }
        const int64_t row = row0 + lg + 4 * i;
        if (row < sh.n && lr < 4) A.rows[(out0 + row) * 4 + lr] = lr == 0 ? c0 : (lr == 1 ? c1 : (lr == 2 ? c2 : c3));
      }
    }
  }
}

// The observed y of a chunk's rows: sum, sum of squares, max, min, zeros.  Thread order, then 256 in index order.
__global__ __launch_bounds__(256) void k_yobs(PpcArgs A) {
  constexpr double INF = __builtin_huge_val();
  __shared__ double red[5][256];
  const int si = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const ShardDev sh = A.shards[A.shard0 + si];
  const int G = ppc_chunks(sh.n);
  if (chunk >= G) return;                            // block-uniform
  const UnitRange groups = draw_chunk_units(draw_units(sh.n, PP_R * PP_W), chunk, G);
  const int64_t r0 = groups.first * (PP_R * PP_W), re = groups.last * (PP_R * PP_W), r1 = re < sh.n ? re : sh.n;
  double v[5] = {0.0, 0.0, -INF, INF, 0.0};
  for (int64_t r = r0 + tid; r < r1; r += 256) {
    const double y = A.family == STK_LINREG ? sh.y[r] : (double)sh.yi[r];
    v[0] += y;
    v[1] = fma(y, y, v[1]);
    v[2] = y > v[2] ? y : v[2];
    v[3] = y < v[3] ? y : v[3];
    v[4] += y == 0.0 ? 1.0 : 0.0;
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) red[k][tid] = v[k];
  __syncthreads();
  if (tid < 5) {
    double x = red[tid][0];
    for (int j = 1; j < 256; ++j) x = ppc_join(tid, x, red[tid][j]);
    A.opart[((size_t)si * A.Gs + chunk) * 8 + tid] = x;
  }
}

// stats[si][s][k] = the chunk partials of draw s joined in chunk order; a draw with NaN replicates has NaN
// extrema.  Block 0 of a shard also joins obs[si][0..4] and sets obs[si][5] = n.
__global__ __launch_bounds__(256) void k_yrep_reduce(PpcArgs A) {
  const int s = blockIdx.x * 256 + threadIdx.x, si = blockIdx.y;
  const ShardDev sh = A.shards[A.shard0 + si];
  const int G = ppc_chunks(sh.n);
  if (A.obs && blockIdx.x == 0 && threadIdx.x < 8) {
    const int k = threadIdx.x;
    double v = 0.0;
    if (k < 5) {
      const double* src = A.opart + (size_t)si * A.Gs * 8 + k;
      v = src[0];
      for (int c = 1; c < G; ++c) v = ppc_join(k, v, src[(size_t)c * 8]);
    } else if (k == 5) {
      v = (double)sh.n;
    }
    A.obs[(size_t)si * 8 + k] = v;
  }
  if (s >= A.S) return;
  const size_t Sp = (size_t)(PP_NS * 16) * A.ntile;
  const double* src = A.partial + (size_t)si * A.Gs * Sp + (size_t)(PP_NS * 16) * (s >> 4) + (s & 15);
  double v[PP_NS];
#pragma unroll
  for (int k = 0; k < PP_NS; ++k) {
    v[k] = src[k * 16];
    for (int c = 1; c < G; ++c) v[k] = ppc_join(k, v[k], src[(size_t)c * Sp + k * 16]);
  }
  if (v[7] > 0.0) v[2] = v[3] = __builtin_nan("");
#pragma unroll
  for (int k = 0; k < PP_NS; ++k) A.stats[((size_t)si * A.S + s) * PP_NS + k] = v[k];
}

template <int FAM, int KF, bool ROWS>
static hipError_t go_yrep(const PpcArgs& A, int d, int nsh, hipStream_t st) {
  const size_t lds = ppc_lds_doubles(d) * sizeof(double);
  auto kern = k_yrep<FAM, KF, ROWS>;
  if (lds > 64 * 1024)
    if (const hipError_t e = allow_big_lds(reinterpret_cast<const void*>(kern))) return e;
  hipLaunchKernelGGL(kern, dim3(A.Gs, nsh), dim3(64 * PP_W), lds, st, A);
  return hipGetLastError();
}

}  // namespace stk

using namespace stk;

bool stk_ppc_supported(int d) { return d >= 1 && d <= 128; }
int stk_ppc_chunks(int64_t n) { return ppc_chunks(n); }
int stk_ppc_rows_per_tile() { return PP_R; }
int stk_ppc_waves() { return PP_W; }
size_t stk_ppc_lds_bytes(int d) { return ppc_lds_doubles(d) * sizeof(double); }
// chunk-partial workspace of one shard: per chunk, 8 x 16 numbers per draw tile and 8 of the observed y
size_t stk_ppc_ws_bytes(int64_t n, int S) {
  return sizeof(double) * ((size_t)(PP_NS * 16) * stk_predictive_tiles(S) + 8) * (size_t)ppc_chunks(n);
}

// Shards [shard0, shard0 + nsh) against the image -> stats [nsh][S][8], obs [nsh][8] (may be null) and, where
// not null, rows and yrep at rowoff[s] (device array of nsh offsets).  partial holds, at the stride Gs >= every
// shard's chunk count, nsh * Gs chunk rows of 128 ceil(S / 16) doubles and then nsh * Gs of 8.  One sweep launch,
// one launch over y and one reduce launch for all of them.
hipError_t stk_launch_ppc(int family, const ShardDev* shards, int shard0, int nsh, int d, int Gs, int S, int draw0,
                          uint64_t seed, const int32_t* streams, const double* img, double* partial, double* stats,
                          double* obs, double* rows, double* yrep, const int64_t* rowoff, hipStream_t st) {
  const int ntile = stk_predictive_tiles(S);
  double* opart = partial + (size_t)nsh * Gs * (PP_NS * 16) * ntile;
  const PpcArgs A{shards, img, partial, opart, stats, obs, rows, yrep, rowoff, streams, seed, family, shard0, Gs, S, ntile, draw0};
  const hipError_t e = draw_dispatch(family, d, [&](auto fam, auto kf) {
    constexpr int F = decltype(fam)::value, K = decltype(kf)::value;
    return rows ? go_yrep<F, K, true>(A, d, nsh, st) : go_yrep<F, K, false>(A, d, nsh, st);
  });
  if (e != hipSuccess) return e;
  if (obs) {
    hipLaunchKernelGGL(k_yobs, dim3(Gs, nsh), dim3(256), 0, st, A);
    if (const hipError_t e2 = hipGetLastError()) return e2;
  }
  hipLaunchKernelGGL(k_yrep_reduce, dim3((unsigned)((S + 255) / 256), nsh), dim3(256), 0, st, A);
  return hipGetLastError();
}
