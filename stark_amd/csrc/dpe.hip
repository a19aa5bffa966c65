// Semiparametric density-product combiner on gfx950 (fp64): the estimator of "Asymptotically exact,
// embarrassingly parallel MCMC" with the kernel covariance h^2 M Sigma_M (DESIGN.md sections 3 and 8).
//
// Prepare (after the combine's own stages gave every shard's mean and precision and Sigma_M):
//   k_dpe_gemm   Y^m = (theta^m - mu_M)^T Linv^T / sqrt(M)  and  Z^m = (theta^m - mu_m)^T W_m, one draw per
//                contiguous row of ldp doubles (pads zero): fp64 MFMA, one wave per 16 x 16 output tile, the
//                contraction run in k order by one accumulator chain, so every output is a fixed-order sum
//                (combine.hip's k_mgemm splits K over 16 waves for K = thousands; here K = p and the outputs
//                are draw-major, and the combine's code object stays as it is)
//   k_dpe_rows   n^m_s = ||y^m_s||^2, g^m_s = 1/2 z^m_s . (theta^m_s - mu_m), the lp__ value of the draw
// Sample:
//   k_dpe_img    one wavefront per chain: independent Metropolis within Gibbs on the index tuple; s_t in
//                registers (coordinate j in lane j & 63, slot j >> 6), indices and accept counts in LDS.  A
//                proposal reads the old and the new row of the image (two independent gathers in flight
//                together), moves s, N and G, and takes ||s'||^2 by lane partial sums and the xor butterfly.
//                Latency-bound by construction: a proposal is one dependent round trip to the image.
//   k_dpe_gemm   theta = mu_M + sqrt(M) L y of the emitted draws (the same kernel, other strides)
// dpe_math.h holds the arithmetic this file shares with the host twin at the bottom.
#include "launchers.h"
#include "dpe_math.h"
#include <vector>

namespace stk {

typedef double dbl4 __attribute__((ext_vector_type(4)));

// O[z][s, j] = scale * sum_k (A[zs][s, k] - cen[zs][k]) B[zs][j, k] + add[j], zs = zmap ? zmap[z] : z
struct DpeGemm {
  const double* A;
  size_t a_z, a_s, a_k;
  const double* cen;      // or null
  size_t cen_z;
  const double* B;        // row j, column k
  size_t b_z;
  int ldb;
  double* O;
  size_t o_z, o_s, o_j;
  double scale;
  const double* add;      // or null
  const int32_t* zmap;    // or null
  int ns, nj, nk, nb;     // rows s, stored columns j < nj, contraction k < nk, rows of B j < nb (else 0)
};

__global__ __launch_bounds__(256) void k_dpe_gemm(DpeGemm L) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int s0 = 16 * (4 * (int)blockIdx.x + w), j0 = 16 * (int)blockIdx.y, z = blockIdx.z;
  if (s0 >= L.ns) return;                            // wave-uniform, no barrier below
  const int zs = L.zmap ? L.zmap[z] : z;
  const double* A = L.A + (size_t)zs * L.a_z;
  const double* cen = L.cen ? L.cen + (size_t)zs * L.cen_z : nullptr;
  const double* B = L.B + (size_t)zs * L.b_z;
  const int sa = s0 + r, jb = j0 + r;
  const bool a_ok = sa < L.ns, b_ok = jb < L.nb;
  dbl4 acc = dbl4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < L.nk; k0 += 4) {
    const int k = k0 + g;
    double a = 0.0, b = 0.0;
    if (k < L.nk) {
      if (a_ok) a = A[(size_t)sa * L.a_s + (size_t)k * L.a_k] - (cen ? cen[k] : 0.0);
      if (b_ok) b = B[(size_t)jb * L.ldb + k];
    }
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
  double* O = L.O + (size_t)z * L.o_z;
  const double add = (L.add && jb < L.nb) ? L.add[jb] : 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int s = s0 + g + 4 * i;
    if (s < L.ns && jb < L.nj) O[(size_t)s * L.o_s + (size_t)jb * L.o_j] = acc[i] * L.scale + add;
  }
}

// per (usable shard z, draw s): n = ||y||^2, g = 1/2 z . (theta - mu_m), lp = the draw's lp__ (lp_row)
__global__ __launch_bounds__(256) void k_dpe_rows(const double* X, const double* mean, const int32_t* zmap, int P, int p,
                                                  int S, int ldp, const double* Y, const double* Z, double* nrm,
                                                  double* gq, double* lpv) {
  const int s = blockIdx.x * 256 + threadIdx.x, z = blockIdx.y;
  if (s >= S) return;
  const int zs = zmap[z];
  const double* y = Y + ((size_t)z * S + s) * ldp;
  const double* zz = Z + ((size_t)z * S + s) * ldp;
  const double* x = X + (size_t)zs * P * S + s;
  const double* mu = mean + (size_t)zs * P;
  double n = 0.0, q = 0.0;
  for (int j = 0; j < p; ++j) {
    n = fma(y[j], y[j], n);
    q = fma(zz[j], x[(size_t)j * S] - mu[j], q);
  }
  nrm[(size_t)z * S + s] = n;
  gq[(size_t)z * S + s] = 0.5 * q;
  if (lpv) lpv[(size_t)z * S + s] = x[(size_t)p * S];
}

struct DpeImg {
  const double *Y, *nrm, *g, *lpv, *lpw;   // lpv / lpw null: no lp__ row
  const DpeCoef* coef;                     // [sweeps]
  double* ydraw;                           // [T][ldp]
  double* lpout;                           // [T] (the output's last row), or null
  unsigned long long* accept;              // [M]
  int32_t* tidx;                           // [K][sweeps][M] or null
  double* tlogw;                           // [K][sweeps] or null
  uint64_t seed;
  uint32_t stream;
  int M, p, ldp, S, T, K, burn, thin, sweeps;
  double inv_m;
};

__device__ __forceinline__ double dpe_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
  return v;
}

template <int NC>
__global__ __launch_bounds__(64) void k_dpe_img(DpeImg A) {
  extern __shared__ int32_t dpe_lds[];
  int32_t* t = dpe_lds;             // [M] the chain's indices
  int32_t* cnt = dpe_lds + A.M;     // [M] accepted proposals
  const int lane = threadIdx.x;
  const uint32_t chain = blockIdx.x;
  const int M = A.M, S = A.S, ldp = A.ldp;
  for (int m = lane; m < M; m += 64) {
    t[m] = (int32_t)dpe_init_index(A.seed, A.stream, chain, (uint32_t)m, (uint32_t)S);
    cnt[m] = 0;
  }
  __syncthreads();
  double s[NC], N = 0.0, G = 0.0;
#pragma unroll
  for (int c = 0; c < NC; ++c) s[c] = 0.0;
  for (int m = 0; m < M; ++m) {
    const size_t row = (size_t)m * S + t[m];
    const double* y = A.Y + row * ldp;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int j = lane + 64 * c;
      s[c] = s[c] + (j < ldp ? y[j] : 0.0);
    }
    N = N + A.nrm[row];
    G = G + A.g[row];
  }
  double q;
  {
    double part = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) part = fma(s[c], s[c], part);
    q = dpe_wave_sum(part);
  }
  for (int r = 0; r < A.sweeps; ++r) {
    const DpeCoef cf = A.coef[r];
    double lw = dpe_logw(N, q, G, A.inv_m, cf);
    for (int m = 0; m < M; ++m) {
      const DpeProposal pr = dpe_proposal(A.seed, A.stream, chain, (uint32_t)r, (uint32_t)m, (uint32_t)S);
      const int old = t[m];
      const size_t ro = (size_t)m * S + old, rn = (size_t)m * S + pr.c;
      const double* yo = A.Y + ro * ldp;
      const double* yn = A.Y + rn * ldp;
      double vo[NC], vn[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int j = lane + 64 * c;
        vo[c] = j < ldp ? yo[j] : 0.0;
        vn[c] = j < ldp ? yn[j] : 0.0;
      }
      const double no = A.nrm[ro], nn = A.nrm[rn], go = A.g[ro], gn = A.g[rn];
      double s2[NC], part = 0.0;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        s2[c] = dpe_move(s[c], vo[c], vn[c]);
        part = fma(s2[c], s2[c], part);
      }
      const double q2 = dpe_wave_sum(part);
      const double N2 = dpe_move(N, no, nn), G2 = dpe_move(G, go, gn);
      const double lw2 = dpe_logw(N2, q2, G2, A.inv_m, cf);
      const bool acc = pr.logu < lw2 - lw;           // wave-uniform: every lane holds the same bits
      __syncthreads();                               // every lane has read t[m]
      if (acc) {
#pragma unroll
        for (int c = 0; c < NC; ++c) s[c] = s2[c];
        N = N2;
        G = G2;
        q = q2;
        lw = lw2;
        if (lane == 0) {
          t[m] = (int32_t)pr.c;
          cnt[m] += 1;
        }
      }
      if (A.tidx && lane == 0) A.tidx[((size_t)chain * A.sweeps + r) * M + m] = acc ? (int32_t)pr.c : old;
    }
    __syncthreads();                                 // the sweep's indices are visible to every lane
    if (A.tlogw && lane == 0) A.tlogw[(size_t)chain * A.sweeps + r] = lw;
    const int e = r + 1 - A.burn;
    if (e > 0 && e % A.thin == 0) {
      const int jd = e / A.thin - 1;
      const long long col = (long long)jd * A.K + chain;
      if (col < A.T) {
        double* yd = A.ydraw + (size_t)col * ldp;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int j = lane + 64 * c;
          if (j < A.p) {
            yd[j] = dpe_draw(s[c], dpe_normal(A.seed, A.stream, chain, (uint32_t)jd, (uint32_t)j), cf);
          } else if (j < ldp) {
            yd[j] = 0.0;
          }
        }
        if (A.lpout && lane == 0) {
          double v = 0.0;
          for (int m = 0; m < M; ++m) v = fma(A.lpw[m], A.lpv[(size_t)m * S + t[m]], v);
          A.lpout[col] = v;
        }
      }
    }
  }
  for (int m = lane; m < M; m += 64) atomicAdd(&A.accept[m], (unsigned long long)cnt[m]);
}

static hipError_t launch_gemm(const DpeGemm& L, int batch, hipStream_t st) {
  const int tiles_s = (L.ns + 15) / 16, tiles_j = (L.nj + 15) / 16;
  hipLaunchKernelGGL(k_dpe_gemm, dim3((tiles_s + 3) / 4, tiles_j, batch), dim3(256), 0, st, L);
  return hipGetLastError();
}

}  // namespace stk

using namespace stk;

int stk_dpe_coords_per_lane(int p) {
  const int need = (dpe_ldp(p) + 63) / 64;
  int nc = 1;
  while (nc < need) nc *= 2;
  return nc;
}
size_t stk_dpe_lds_bytes(int M) { return sizeof(int32_t) * 2 * (size_t)M; }

// X [nshards][P][S], mean [nshards][P], W [nshards][P][P] (the combine's stages); zmap [M] the usable shards;
// mu_M [p], Linv [p][p] -> Y, nrm, g, lpv ([M][S][ldp], [M][S] x 3; lpv null without an lp__ row); Z: [M][S][ldp] scratch
hipError_t stk_launch_dpe_image(const double* X, const double* mean, const double* W, const int32_t* zmap, int M, int P,
                                int p, int S, const double* mu, const double* Linv, double* Y, double* Z, double* nrm,
                                double* g, double* lpv, hipStream_t st) {
  const int ldp = dpe_ldp(p);
  const size_t per = (size_t)P * S, img = (size_t)S * ldp;
  DpeGemm wh{X, per, 1, (size_t)S, mu, 0, Linv, 0, p, Y, img, (size_t)ldp, 1, 1.0 / sqrt((double)M), nullptr, zmap,
             S, ldp, p, p};
  hipError_t e = launch_gemm(wh, M, st);
  if (e != hipSuccess) return e;
  DpeGemm mh{X, per, 1, (size_t)S, mean, (size_t)P, W, (size_t)P * P, P, Z, img, (size_t)ldp, 1, 1.0, nullptr, zmap,
             S, ldp, p, p};
  e = launch_gemm(mh, M, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_dpe_rows, dim3((S + 255) / 256, M), dim3(256), 0, st, X, mean, zmap, P, p, S, ldp, Y, Z, nrm, g,
                     lpv);
  return hipGetLastError();
}

// the chains: ydraw [T][ldp], lpout [T] or null, accept [M] (added to), trace or null
hipError_t stk_launch_dpe_chains(const StkDpeChains& c, hipStream_t st) {
  DpeImg A{c.Y, c.nrm, c.g, c.lpv, c.lpw, (const DpeCoef*)c.coef, c.ydraw, c.lpout, c.accept, c.tidx, c.tlogw,
           c.seed, c.stream, c.M, c.p, dpe_ldp(c.p), c.S, c.T, c.K, c.burn, c.thin, c.sweeps, 1.0 / (double)c.M};
  const size_t lds = stk_dpe_lds_bytes(c.M);
  switch (stk_dpe_coords_per_lane(c.p)) {
#define STK_DPE(N) \
  case N: hipLaunchKernelGGL(k_dpe_img<N>, dim3(c.K), dim3(64), lds, st, A); break;
    STK_DPE(1) STK_DPE(2) STK_DPE(4) STK_DPE(8) STK_DPE(16)
#undef STK_DPE
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// theta [p][T] = mu_M + sqrt(M) L y for the emitted draws ydraw [T][ldp]; out has row stride T
hipError_t stk_launch_dpe_map(const double* ydraw, const double* L, const double* mu, int M, int p, int T, double* out,
                              hipStream_t st) {
  const int ldp = dpe_ldp(p);
  DpeGemm mp{ydraw, 0, (size_t)ldp, 1, nullptr, 0, L, 0, p, out, 0, 1, (size_t)T, sqrt((double)M), mu, nullptr,
             T, p, p, p};
  return launch_gemm(mp, 1, st);
}

// ---------------------------------------------------------------- host twin
// The chains of k_dpe_img on host arrays: dpe_math.h's arithmetic, the lanes' partial sums and the
// butterfly spelled out, the same sum orders.  out [p (+ 1)][T].
void stk_dpe_chains_host(const StkDpeChains& c, const double* mu, const double* L, double* out) {
  const int M = c.M, p = c.p, S = c.S, ldp = dpe_ldp(p), NC = (ldp + 63) / 64, W = 64 * NC;
  const DpeCoef* coef = (const DpeCoef*)c.coef;
  const double inv_m = 1.0 / (double)M, rtm = sqrt((double)M);
  std::vector<double> s(W), s2(W), yd(p);
  std::vector<int32_t> t(M);
  auto at = [&](const double* row, int j) { return j < ldp ? row[j] : 0.0; };
  auto normsq = [&](const std::vector<double>& v) {
    double part[64];
    for (int l = 0; l < 64; ++l) {
      double a = 0.0;
      for (int cc = 0; cc < NC; ++cc) a = fma(v[l + 64 * cc], v[l + 64 * cc], a);
      part[l] = a;
    }
    return dpe_butterfly_host(part);
  };
  for (int k = 0; k < c.K; ++k) {
    const uint32_t chain = (uint32_t)k;
    for (int m = 0; m < M; ++m) t[m] = (int32_t)dpe_init_index(c.seed, c.stream, chain, (uint32_t)m, (uint32_t)S);
    std::fill(s.begin(), s.end(), 0.0);
    double N = 0.0, G = 0.0;
    for (int m = 0; m < M; ++m) {
      const size_t row = (size_t)m * S + t[m];
      for (int j = 0; j < W; ++j) s[j] = s[j] + at(c.Y + row * ldp, j);
      N = N + c.nrm[row];
      G = G + c.g[row];
    }
    double q = normsq(s);
    for (int r = 0; r < c.sweeps; ++r) {
      const DpeCoef cf = coef[r];
      double lw = dpe_logw(N, q, G, inv_m, cf);
      for (int m = 0; m < M; ++m) {
        const DpeProposal pr = dpe_proposal(c.seed, c.stream, chain, (uint32_t)r, (uint32_t)m, (uint32_t)S);
        const int old = t[m];
        const size_t ro = (size_t)m * S + old, rn = (size_t)m * S + pr.c;
        for (int j = 0; j < W; ++j) s2[j] = dpe_move(s[j], at(c.Y + ro * ldp, j), at(c.Y + rn * ldp, j));
        const double q2 = normsq(s2);
        const double N2 = dpe_move(N, c.nrm[ro], c.nrm[rn]), G2 = dpe_move(G, c.g[ro], c.g[rn]);
        const double lw2 = dpe_logw(N2, q2, G2, inv_m, cf);
        const bool acc = pr.logu < lw2 - lw;
        if (acc) {
          s.swap(s2);
          N = N2;
          G = G2;
          q = q2;
          lw = lw2;
          t[m] = (int32_t)pr.c;
          c.accept[m] += 1;
        }
        if (c.tidx) c.tidx[((size_t)k * c.sweeps + r) * M + m] = t[m];
      }
      if (c.tlogw) c.tlogw[(size_t)k * c.sweeps + r] = lw;
      const int e = r + 1 - c.burn;
      if (e > 0 && e % c.thin == 0) {
        const int jd = e / c.thin - 1;
        const long long col = (long long)jd * c.K + k;
        if (col < c.T) {
          for (int j = 0; j < p; ++j) yd[j] = dpe_draw(s[j], dpe_normal(c.seed, c.stream, chain, (uint32_t)jd, (uint32_t)j), cf);
          for (int i = 0; i < p; ++i) {
            double v = 0.0;
            for (int j = 0; j <= i; ++j) v = fma(L[(size_t)i * p + j], yd[j], v);
            out[(size_t)i * c.T + col] = fma(rtm, v, mu[i]);
          }
          if (c.lpv) {
            double v = 0.0;
            for (int m = 0; m < M; ++m) v = fma(c.lpw[m], c.lpv[(size_t)m * S + t[m]], v);
            out[(size_t)p * c.T + col] = v;
          }
        }
      }
    }
  }
}
