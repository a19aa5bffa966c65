// The analytic Hessian sweep (regression families, 1 <= d <= 128): the Hessian of Stan's
// log_prob<propto, jacobian> of a shard at ONE point, with respect to the unconstrained parameters,
// in a single pass over the shard's rows on the fp64 MFMA.  No reference counterpart: it supersedes
// the central difference of the gradient in tools/laplace.py on the product path (per-shard Laplace
// fits, the exact consensus weights W_s = -H_s; DESIGN.md sections 3 and 8).
//
// Every family's Hessian is one weighted Gram matrix of the augmented rows
//   xt_i = [x_i1 .. x_id | 1 | r_i | 0 ..]      (C = d + 2 live columns, padded to 16 NT)
//   Gram = sum_i xt_i^T w_i xt_i                eta_i = alpha + x_i . beta
//   logistic  w_i = s(eta_i)(1 - s(eta_i)) = t / (1 + t)^2, t = exp(-|eta_i|)   (r_i = 0)
//             -- a large |eta| underflows to w = 0, never NaN
//   poisson   w_i = mu_i = exp(eta_i)                                            (r_i = 0)
//   linear    w_i = 1, r_i = y_i - eta_i: the r column makes X~^T r and sum r^2 part of the same Gram
// and k_hessian_reduce turns the Gram into H (parameter a sits in column d for alpha, a - 1 for
// beta_a, d + 1 for u = log sigma):
//   logistic, poisson   H = -Gram
//   linear              H_tt = -e^-2u Gram_tt, H_tu = -2 e^-2u Gram_t,r, H_uu = -2 e^-2u Gram_r,r
//   priors              -1/s^2 on the diagonal entries the normal(0, s) priors cover
// The geometry is the same for the three families (the r column is zero and costs logistic / poisson
// one more column tile only at d = 15 mod 16), so stk_hessian_launch_info is a function of (n, d).
//
// Workgroup = 4 waves that share one 16-row LDS tile; a shard is cut into G chunks of whole 16-row
// tiles that depend only on n.  Per tile:
//   load      wave w brings rows 4w .. 4w + 3 from HBM (nontemporal: X is read once) into registers
//             one tile ahead and parks them, with the ones column, in one half of a double buffer;
//   weights   16 lanes per row form eta (fixed-order partial sums, xor butterfly), then w_i, and
//             write the scaled copy w_i xt_i (linear: the r column) next to the tile;
//   Gram      the NT (NT + 1) / 2 upper-triangle 16 x 16 tiles are dealt round-robin to the 4 waves
//             (<= 12 accumulator tiles = 96 VGPRs at NT = 9); tile (I, J) takes 4 MFMAs of k = 4 rows:
//             lane (r, g) supplies A = xt[4s + g][16 I + r] and B = (w xt)[4s + g][16 J + r].
//             The LDS row stride is 16 mod 32 doubles, so the four row groups of a read fall on
//             different bank halves.
// The weights take the library exp, one call per ROW (the sweeps' table exp serves one per row and
// chain; here it would buy nothing, cost 8 KB of LDS -- the second workgroup per CU at NT >= 8 --
// and its clamp turns a NaN eta into a finite mu, which this entry point must not do).
// Rows past the shard's end are zero rows with w = 0.  Every chunk writes its partial tiles;
// k_hessian_reduce sums them in chunk order and mirrors the upper triangle (inside the diagonal
// tiles too), so H is symmetric to the bit and bitwise independent of how many shards share a
// launch and of which GPU runs a shard.  A NaN eta or an overflowing mu gives non-finite entries.
#include "launchers.h"
#include <math.h>
#include <algorithm>

namespace stk {

typedef double hdbl4 __attribute__((ext_vector_type(4)));

constexpr int HS_R = 16;          // rows per tile = 4 MFMA k-steps
constexpr int HS_W = 4;           // waves per block
constexpr int HS_TPC = 32;        // 16-row tiles per chunk before the chunk count saturates
constexpr int HS_GMAX = 256;      // chunks per shard at most

__host__ __device__ constexpr int hess_nt(int d) { return (d + 2 + 15) / 16; }
__host__ __device__ constexpr int hess_ld(int nt) { return (nt & 1) ? 16 * nt : 16 * nt + 16; }
__host__ __device__ inline int hess_chunks(int64_t n) {
  const int64_t nt = (n + HS_R - 1) / HS_R, g = (nt + HS_TPC - 1) / HS_TPC;
  return (int)(g < 1 ? 1 : (g > HS_GMAX ? HS_GMAX : g));
}
__host__ __device__ constexpr size_t hess_lds_doubles(int nt) { return (size_t)4 * HS_R * hess_ld(nt) + hess_ld(nt) + 2 * HS_R; }

struct HessArgs {
  const ShardDev* shards;
  const double* q;        // [nsh][D] one point per shard of the launch
  double* partial;        // [nsh][Gs][NP][256] chunk-partial tiles
  double* hess;           // [nsh][D][D]
  int family, shard0, Gs, D;
};

template <int NT>
__global__ __launch_bounds__(64 * HS_W, 2) void k_hessian(HessArgs A) {
  constexpr int NP = NT * (NT + 1) / 2, PPW = (NP + HS_W - 1) / HS_W, LD = hess_ld(NT), TILE = HS_R * LD;
  const int si = blockIdx.y, chunk = blockIdx.x;
  const ShardDev sh = A.shards[A.shard0 + si];
  const int G = hess_chunks(sh.n);
  if (chunk >= G) return;                            // block-uniform
  const int d = sh.d;
  const bool LIN = A.family == STK_LINREG, LOGI = A.family == STK_LOGREG;
  const int tid = threadIdx.x, lane = tid & 63, w = uniform_int(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4;

  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* const xs = lds;                            // [2][16][LD] the tile
  double* const xw = lds + 2 * TILE;                 // [2][16][LD] w . tile
  double* const bs = lds + 4 * TILE;                 // [LD] beta, alpha at column d
  double* const ys = bs + LD;                        // [2][16] y (linear)
  for (int i = tid; i < 4 * TILE + LD + 2 * HS_R; i += 64 * HS_W) lds[i] = 0.0;
  __syncthreads();
  const double* qs = A.q + (size_t)si * A.D;
  for (int c = tid; c <= d; c += 64 * HS_W) bs[c] = c < d ? qs[1 + c] : qs[0];
  __syncthreads();

  const int64_t nt = (sh.n + HS_R - 1) / HS_R;
  const int64_t t0 = nt * chunk / G, t1 = nt * (chunk + 1) / G;
  const gptr_t<double> xg = gp(sh.x);
  double pre[4][2], ypre = 0.0;
  auto fetch = [&](int64_t t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t row = t * HS_R + 4 * w + i;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int col = lane + 64 * h;
        pre[i][h] = (row < sh.n && col < d) ? __builtin_nontemporal_load(xg + row * d + col) : 0.0;
      }
    }
    if (LIN && tid < HS_R) {
      const int64_t row = t * HS_R + tid;
      ypre = row < sh.n ? sh.y[row] : 0.0;
    }
  };

  // the wave's tile pairs p = w, w + 4, ...: (I, J), I <= J, row by row
  int offA[PPW], offB[PPW];
#pragma unroll
  for (int pi = 0; pi < PPW; ++pi) {
    int p = w + HS_W * pi, I = 0;
    if (p < NP) {
      while (p >= NT - I) { p -= NT - I; ++I; }
      offA[pi] = 16 * I;
      offB[pi] = 16 * (I + p);
    } else {
      offA[pi] = offB[pi] = -1;
    }
  }
  hdbl4 acc[PPW];
#pragma unroll
  for (int pi = 0; pi < PPW; ++pi) acc[pi] = hdbl4{0.0, 0.0, 0.0, 0.0};

  fetch(t0);
  for (int64_t t = t0; t < t1; ++t) {
    const int buf = (int)((t - t0) & 1);
    double* const X = xs + buf * TILE;
    double* const XW = LIN ? X : xw + buf * TILE;
    // ---- park the prefetched rows (columns 0 .. d - 1, the ones column d); columns past d + 1 stay 0
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rowl = 4 * w + i;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int col = lane + 64 * h;
        if (col < d) X[rowl * LD + col] = pre[i][h];
      }
      if (lane == 0) X[rowl * LD + d] = (t * HS_R + rowl < sh.n) ? 1.0 : 0.0;
    }
    if (LIN && tid < HS_R) ys[buf * HS_R + tid] = ypre;
    if (t + 1 < t1) fetch(t + 1);
    __syncthreads();
    // ---- eta and the weight of row tid >> 4, 16 lanes per row
    {
      const int rowl = tid >> 4, j = tid & 15;
      const bool live = t * HS_R + rowl < sh.n;
      double xv[NT], e = 0.0;
#pragma unroll
      for (int m = 0; m < NT; ++m) {
        const int c = j + 16 * m;
        xv[m] = X[rowl * LD + c];
        if (c <= d) e = fma(xv[m], bs[c], e);
      }
      e += __shfl_xor(e, 8);
      e += __shfl_xor(e, 4);
      e += __shfl_xor(e, 2);
      e += __shfl_xor(e, 1);
      if (LIN) {
        if (j == 0) X[rowl * LD + d + 1] = live ? ys[buf * HS_R + rowl] - e : 0.0;
      } else {
        double wgt;
        if (LOGI) {
          const double tt = exp(-fabs(e));
          wgt = tt / ((1.0 + tt) * (1.0 + tt));
        } else {
          wgt = exp(e);
        }
        if (!live) wgt = 0.0;
#pragma unroll
        for (int m = 0; m < NT; ++m) {
          const int c = j + 16 * m;
          if (c <= d) XW[rowl * LD + c] = wgt * xv[m];
        }
      }
    }
    __syncthreads();
    // ---- Gram tiles
#pragma unroll
    for (int pi = 0; pi < PPW; ++pi) {
      if (offA[pi] >= 0) {                             // wave-uniform
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double a = X[(4 * s + lg) * LD + offA[pi] + lr];
          const double b = XW[(4 * s + lg) * LD + offB[pi] + lr];
          acc[pi] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[pi], 0, 0, 0);
        }
      }
    }
  }
  double* out = A.partial + ((size_t)si * A.Gs + chunk) * NP * 256;
#pragma unroll
  for (int pi = 0; pi < PPW; ++pi) {
    const int p = w + HS_W * pi;
    if (p < NP) {
#pragma unroll
      for (int i = 0; i < 4; ++i) out[p * 256 + (lg + 4 * i) * 16 + lr] = acc[pi][i];
    }
  }
}

// H[a][b] of every shard of the launch: the chunk partials of Gram entry (column of a, column of b),
// taken from the upper triangle, summed in chunk order; then the family's scale and the priors.
__global__ __launch_bounds__(256) void k_hessian_reduce(HessArgs A, int NT) {
  const int si = blockIdx.y;
  const ShardDev sh = A.shards[A.shard0 + si];
  const int d = sh.d, D = sh.D, G = hess_chunks(sh.n), NP = NT * (NT + 1) / 2;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= D * D) return;
  const int a = idx / D, b = idx - a * D;
  int ca = a == 0 ? d : (a <= d ? a - 1 : d + 1), cb = b == 0 ? d : (b <= d ? b - 1 : d + 1);
  if (ca > cb) { const int t = ca; ca = cb; cb = t; }
  const int I = ca >> 4, J = cb >> 4;
  const int p = I * NT - I * (I - 1) / 2 + (J - I);
  const double* src = A.partial + (size_t)si * A.Gs * NP * 256 + (size_t)p * 256 + (ca & 15) * 16 + (cb & 15);
  double v = src[0];
  for (int k = 1; k < G; ++k) v += src[(size_t)k * NP * 256];
  if (A.family == STK_LINREG) {
    const double s = exp(-2.0 * A.q[(size_t)si * A.D + d + 1]);
    v = -((a == d + 1 || b == d + 1) ? 2.0 : 1.0) * s * v;
  } else {
    v = -v;
  }
  if (a == b) {
    if (a == 0) v -= sh.pa;
    else if (a <= d) v -= sh.pb;
  }
  A.hess[((size_t)si * D + a) * D + b] = v;
}

template <int NT>
static hipError_t go_hessian(const HessArgs& A, int gmax, int nsh, hipStream_t st) {
  const size_t lds = hess_lds_doubles(NT) * sizeof(double);
  if (lds > 64 * 1024)
    if (const hipError_t e = allow_big_lds(reinterpret_cast<const void*>(&k_hessian<NT>))) return e;
  hipLaunchKernelGGL(k_hessian<NT>, dim3(gmax, nsh), dim3(64 * HS_W), lds, st, A);
  return hipGetLastError();
}

}  // namespace stk

using namespace stk;

bool stk_hessian_supported(int d) { return d >= 1 && d <= 128; }
int stk_hessian_chunks(int64_t n) { return hess_chunks(n); }
int stk_hessian_rows_per_tile() { return HS_R; }
int stk_hessian_waves() { return HS_W; }
size_t stk_hessian_lds_bytes(int d) { return hess_lds_doubles(hess_nt(d)) * sizeof(double); }
size_t stk_hessian_ws_bytes(int64_t n, int d) {
  const int nt = hess_nt(d);
  return sizeof(double) * 256 * (size_t)(nt * (nt + 1) / 2) * hess_chunks(n);
}

// Shards [shard0, shard0 + nsh) at q [nsh][D] -> hess [nsh][D][D]; partial holds nsh * Gs chunks,
// Gs >= every shard's chunk count.  One sweep launch and one reduce launch for all of them.
hipError_t stk_launch_hessian(int family, const ShardDev* shards, int shard0, int nsh, int d, int D, int Gs,
                              const double* q, double* partial, double* hess, hipStream_t st) {
  const HessArgs A{shards, q, partial, hess, family, shard0, Gs, D};
  const int nt = hess_nt(d);
  hipError_t e = hipErrorInvalidValue;
  switch (nt) {
#define STK_HS(N) case N: e = go_hessian<N>(A, Gs, nsh, st); break;
    STK_HS(1) STK_HS(2) STK_HS(3) STK_HS(4) STK_HS(5) STK_HS(6) STK_HS(7) STK_HS(8) STK_HS(9)
#undef STK_HS
  }
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_hessian_reduce, dim3((D * D + 255) / 256, nsh), dim3(256), 0, st, A, nt);
  return hipGetLastError();
}
