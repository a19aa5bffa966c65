// The regression log-density + gradient sweep over a SPARSE shard for gfx950: the design matrix as padded rows
// (ELL: idx[n][K] int32, val[n][K] double, K the shard's longest row, short rows padded with (0, 0.0)), 12 K bytes
// per row in place of the dense sweeps' 8 d.  One pass over a chunk of rows serves the C chains of a batch:
//   forward   eta[r][c] = alpha_c + sum_k val[r][k] beta_c[idx[r][k]]      thread = (row, chain), beta in LDS as [d][C]
//   residual  the dense sweeps' own (sweep_common.h), the exp table where fam_exp_table says so
//   backward  G[idx[r][k]][c] += d eta[r][c] val[r][k]                     G in LDS as [d][C], plain read-add-write
// The backward is a scatter, and it is kept bit-reproducible without a floating-point atomic: a block keeps GC
// private copies of G (as many of 4, 2, 1 as its LDS holds); copy q takes the tile's rows r = q (mod GC) in row order,
// and the 4 / GC waves that share a copy each own the columns j = o (mod 4 / GC), so that no two waves ever touch one
// element, a wave's updates of an element happen in row order (LDS operations of one wave complete in order), and the
// lanes of one wave-instruction hold entries of ONE row, whose columns are distinct.  A padded slot (value 0) is
// skipped in the backward: several of a row's slots may name column 0.  The copies are added in copy order at the end.
// So a chunk's partial row depends on the chunk's rows alone; chunks are a function of n alone and k_sweep_reduce
// (sweep.hip) adds them in chunk order, unchanged.
//
// A tile's entries are staged in LDS (coalesced 4- and 8-byte loads into registers one tile ahead, then ds_write)
// when 12 K T bytes fit the stage; a shard with longer rows reads them from global memory where it needs them -- the
// same arithmetic in the same order, so the same bits.
//
// What bounds it: the latency of LDS, not HBM.  Every (entry, chain) pair costs a beta read in the forward and a
// dependent G read and G write in the backward, one such chain per wave at two waves per SIMD; measured 4.3 x faster
// than the dense sweep at d = 1024, K = 16 and 2.4 x slower at d = 128, K = 8 (DESIGN.md "Sparse design matrices").
//
// The library compiles this file once per STK_SWEEP_TU (sweep_common.h), as the dense kernel files.
#include "sweep_common.h"
#include "launchers.h"
#include <algorithm>

namespace stk {

constexpr int SP_NT = 256, SP_NW = 4;        // threads and waves per block
[[maybe_unused]] constexpr int SP_D16_MAX = 512;   // 16 chains: beta and G [d][16] fit the CU's LDS next to the table up to here
constexpr int SP_STAGE = 16 * 1024;          // bytes of the entry stage
[[maybe_unused]] constexpr int SP_CHUNK_ROWS = 2048;   // rows per chunk, at least (beta in, G out: 16 d C bytes per chunk)
constexpr int SP_NV = (SP_STAGE / 12 + SP_NT - 1) / SP_NT;   // staged entries per thread

__host__ __device__ constexpr int sp_passes(int C) { return C > 4 ? C / 4 : 1; }                   // forward passes per tile
__host__ __device__ constexpr int sp_tile_rows(int C) { return SP_NT / C * sp_passes(C); }         // 64, 64, 64, 128, 256 at C = 16 .. 1
// d eta of a tile [T][C], and at the end the three scalar sums of every thread
__host__ __device__ constexpr int sp_scratch(int C) { return sp_tile_rows(C) * C > 3 * SP_NT ? sp_tile_rows(C) * C : 3 * SP_NT; }
__host__ __device__ constexpr size_t sp_lds_bytes(int d, int C, int copies) {
  return sizeof(double) * ((size_t)d * C * (1 + copies) + sp_scratch(C) + EX_TAB) + SP_STAGE;
}
// Private copies of G per block: the most that leave two blocks per CU; else the most that fit one.
__host__ __device__ constexpr int sp_copies(int d, int C) {
  for (int g = SP_NW; g > 1; g >>= 1)
    if (sp_lds_bytes(d, C, g) <= BIG_LDS_BYTES / 2) return g;
  for (int g = SP_NW; g > 1; g >>= 1)
    if (sp_lds_bytes(d, C, g) <= BIG_LDS_BYTES) return g;
  return 1;
}

template <int FAM, int C>
__global__ __launch_bounds__(SP_NT) void k_sweep_sp(SweepArgs A, const SpShardDev* sps) {
  constexpr int NT = SP_NT, RP = NT / C, P = sp_passes(C), T = RP * P, EPW = 64 / C;
  static_assert(fam_known(FAM), "k_sweep_sp: unknown family");
  static_assert(C == 1 || C == 2 || C == 4 || C == 8 || C == 16, "k_sweep_sp: C is 1, 2, 4, 8 or 16");
  constexpr bool LOGI = FAM == STK_LOGREG, NB = FAM == STK_NEGBIN, ST = FAM == STK_STUDENT;
  using yv_t = typename std::conditional<fam_yint(FAM), int32_t, double>::type;
  const int shard = A.shard0 + blockIdx.x / A.G;
  const int chunk = blockIdx.x % A.G;
  if (A.req_step && A.req_step[shard] != A.step_id - 1) return;
  if (A.ran && chunk == 0 && threadIdx.x == 0) atomicAdd(&A.ran[A.step_id & 63], 1);
  const ShardDev sh = A.shards[shard];
  const SpShardDev sp = sps[shard];
  const int d = sh.d, K = sp.K, tid = threadIdx.x, lane = tid & 63, w = uniform_int(tid >> 6);
  const int c = tid % C, r = tid / C;            // this thread's chain (also lane % C) and its row of a forward pass
  const int64_t r0 = sh.n * chunk / A.G, r1 = sh.n * (chunk + 1) / A.G;
  const gptr_t<int32_t> IDX = gp(sp.idx);
  const gptr_t<double> VAL = gp(sp.val);
  const gptr_t<yv_t> Y = (gptr_t<yv_t>)(fam_yint(FAM) ? (const void*)sh.yi : (const void*)fam_ydouble<FAM>(sh));
  const int GC = sp_copies(d, C), OW = SP_NW / GC;   // copies of G; waves that share one

  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int dC = d * C;
  double* Bs = lds;                              // [d][C] beta
  double* Gs = Bs + dC;                          // [GC][d][C]
  double* Rs = Gs + (size_t)GC * dC;             // [T][C] d eta
  double* tab = Rs + sp_scratch(C);              // the exp table (the families that take one)
  double* sV = tab + (fam_exp_table(FAM) ? EX_TAB : 0);   // the stage: values [T K], then columns [T K]
  const bool staged = (int64_t)T * K * 12 <= A.LD;
  int32_t* sI = reinterpret_cast<int32_t*>(sV + (staged ? T * K : 0));

  if constexpr (fam_exp_table(FAM)) exp_table_init(tab);
  for (int i = tid; i < dC; i += NT) {
    const int cc = i / d, j = i - cc * d;
    Bs[j * C + cc] = A.q[chain_row(A, shard, cc) * A.Dp + 1 + j];
  }
  for (int i = tid; i < GC * dC; i += NT) Gs[i] = 0.0;
  const double* qc = A.q + chain_row(A, shard, c) * A.Dp;
  const double alpha = qc[0];
  double inv_s = 0.0, nbphi = 0.0;
  if constexpr (fam_inv_sigma(FAM) || FAM == STK_GAMMA || NB) inv_s = fam_chain_scalar<FAM>(qc[d + 1]);
  if constexpr (NB) nbphi = exp(inv_s);
  double nu = 0.0, nu1 = 0.0, inv_nu = 0.0;
  if constexpr (ST) nu = shard_nu(sh), nu1 = nu + 1.0, inv_nu = 1.0 / nu;

  double lm = 0.0, ss = 0.0, ll = 0.0, ga = 0.0;   // as k_sweep16w: logistic lp pieces lm, ss (the running product), ll;
  int since = 0;                                   // linear lm = sum z^2; the others lm = lp; ss the third sum
  int32_t pi[SP_NV];
  double pv[SP_NV];
  auto fetch = [&](int64_t ts) {                   // a tile's entries into registers: contiguous in both arrays
    const int64_t base = ts * K;
    const int ne = (int)std::min<int64_t>(T, r1 - ts) * K;
#pragma unroll
    for (int v = 0; v < SP_NV; ++v) {
      const int i = tid + NT * v;
      if (i < ne) {
        pi[v] = IDX[base + i];
        pv[v] = VAL[base + i];
      }
    }
  };
  if (staged && r0 < r1) fetch(r0);
  __syncthreads();

  for (int64_t t0 = r0; t0 < r1; t0 += T) {
    const int rows = (int)std::min<int64_t>(T, r1 - t0);
    if (staged) {
      const int ne = rows * K;
#pragma unroll
      for (int v = 0; v < SP_NV; ++v) {
        const int i = tid + NT * v;
        if (i < ne) {
          sI[i] = pi[v];
          sV[i] = pv[v];
        }
      }
      __syncthreads();
      if (t0 + T < r1) fetch(t0 + T);
    }
    // ---- forward + residual: P passes of 256 / C rows.  The P rows of a thread are P independent fma chains over
    // k (a row past the tile's end repeats the last row and is dropped below): no branch around the loads.
    double etap[P];
    int rb[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      rb[p] = std::min(p * RP + r, rows - 1) * K;
      etap[p] = alpha;
    }
    if (staged) {
#pragma unroll 2
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int p = 0; p < P; ++p) etap[p] = fma(sV[rb[p] + k], Bs[sI[rb[p] + k] * C + c], etap[p]);
    } else {
      const gptr_t<int32_t> ti = IDX + t0 * K;
      const gptr_t<double> tv = VAL + t0 * K;
#pragma unroll 2
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int p = 0; p < P; ++p) etap[p] = fma(tv[rb[p] + k], Bs[ti[rb[p] + k] * C + c], etap[p]);
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int rl = p * RP + r;
      double de = 0.0;
      if (rl < rows) {
        const int64_t row = t0 + rl;
        const double eta = etap[p];
        const yv_t y = Y[row];
        if constexpr (LOGI) {
          de = logit_resid4(eta, (uint32_t)y, tab, lm, ss);
        } else if constexpr (NB) {
          de = negbin_resid(eta, y, inv_s, nbphi, tab, lm, ss);
        } else if constexpr (ST) {
          de = student_resid(eta, y, inv_s, nu, nu1, inv_nu, lm, ss);
        } else if constexpr (FAM == STK_GAMMA) {
          de = gamma_resid(eta, y, inv_s, tab, lm);
        } else if constexpr (FAM == STK_POISSON) {
          de = pois_resid(eta, y, tab, lm);
        } else {
          const double z = (y - eta) * inv_s;
          lm = fma(z, z, lm);
          de = z * inv_s;
        }
        ga += de;
      }
      Rs[rl * C + c] = de;
    }
    if constexpr (LOGI) {   // at most 128 + P factors of at most 2 in the running product between flushes
      since += P;
      if (since >= 128) {
        ll += log1p(ss);
        ss = 0.0;
        since = 0;
      }
    }
    __syncthreads();
    // ---- backward: wave (copy q, owner o) takes rows q, q + GC, ... and the columns j = o (mod OW); its lanes are
    // (slot e of the row's next EPW, chain c).  The next step's entry is read before this step's G is touched, and no
    // load sits behind a branch: a slot past the row's K or the tile's rows reads the nearest one that exists and takes
    // the value 0, which is skipped like a padded slot; only the write is predicated (a lane must not write back a
    // column that another wave owns).
    if (K > 0) {
      const int q = w % GC, o = w / GC, e = lane / C;
      double* G = Gs + (size_t)q * dC;
      auto walk = [&](auto load) {   // load(row of the tile, slot, j, v): an entry that exists
        auto entry = [&](int rr, int k0, int& j, double& v, double& rd) {
          const int k = k0 + e, rc = std::min(rr, rows - 1);
          load(rc, std::min(k, K - 1), j, v);
          rd = Rs[rc * C + c];
          v = (rr < rows && k < K) ? v : 0.0;
        };
        int jn;
        double vn, rn;
        entry(q, 0, jn, vn, rn);
        for (int rr = q; rr < rows; rr += GC) {
          for (int k0 = 0; k0 < K; k0 += EPW) {
            const int j = jn;
            const double v = vn, rd = rn;
            const bool last = k0 + EPW >= K;
            entry(last ? rr + GC : rr, last ? 0 : k0 + EPW, jn, vn, rn);
            const double g = fma(rd, v, G[j * C + c]);
            if (v != 0.0 && (j & (OW - 1)) == o) G[j * C + c] = g;
          }
        }
      };
      if (staged) {
        walk([&](int rr, int k, int& j, double& v) {
          j = sI[rr * K + k];
          v = sV[rr * K + k];
        });
      } else {
        walk([&](int rr, int k, int& j, double& v) {
          const int64_t i = (t0 + rr) * K + k;
          j = IDX[i];
          v = VAL[i];
        });
      }
    }
    __syncthreads();
  }

  // ---- the chunk's partial row per chain: the copies of G added in copy order, then the scalar sums of the
  // 256 / C threads of a chain in thread order
  double lpa;
  if constexpr (LOGI) {   // the residual returned -dv: negate the gradient sums once
    lpa = 0.5 * lm - (ll + log1p(ss));
    ga = -ga;
  } else {
    lpa = lm;
  }
  double* out = A.partial + ((size_t)shard * A.Gs + chunk) * C * A.PW;
  for (int i = tid; i < dC; i += NT) {
    const int cc = i / d, j = i - cc * d;
    double v = Gs[j * C + cc];
    for (int g = 1; g < GC; ++g) v += Gs[(size_t)g * dC + j * C + cc];
    out[(size_t)cc * A.PW + 1 + j] = LOGI ? -v : v;
  }
  double* red = Rs;        // [3][NT]; the last tile's d eta is done with (the loop ends on a barrier)
  red[tid] = lpa;
  red[NT + tid] = ga;
  red[2 * NT + tid] = ss;
  __syncthreads();
  if (tid < 3 * C) {
    const int cc = tid % C, kind = tid / C;
    if (kind < 2 || fam_sum3(FAM)) {
      const double* src = red + kind * NT + cc;
      double v = 0.0;
      for (int i = 0; i < RP; ++i) v += src[i * C];
      out[(size_t)cc * A.PW + (kind == 0 ? d + 1 : kind == 1 ? 0 : d + 2)] = v;
    }
  }
}

}  // namespace stk

using namespace stk;

#ifdef STK_SWEEP_BASE
// The single-launch chain counts the sparse sweep covers at d covariates: no 64-chain pass, and 16 while beta and G
// [d][16] fit the CU's LDS next to the exp table.
bool stk_sweep_sparse_supported(int C, int d) {
  if (!(C == 1 || C == 2 || C == 4 || C == 8 || C == 16)) return false;
  return d >= 1 && d <= 1024 && (C < 16 || d <= SP_D16_MAX);
}

// Kind 7's shape over n rows of d covariates for C chains.  The chunks are a function of n alone; K is not an
// argument: the kernel reads it from the shard, and whether a tile's entries fit the stage changes no bit.
SweepLaunch stk_sweep_plan_sparse(int64_t n, int d, int C) {
  SweepLaunch p{};
  p.C = C;
  p.d = d;
  if (n < 1 || !stk_sweep_sparse_supported(C, d)) return p;
  p.kind = SWEEP_SPARSE;
  p.T = sp_tile_rows(C);
  p.G = (int)std::max<int64_t>(1, std::min<int64_t>(512, (n + SP_CHUNK_ROWS - 1) / SP_CHUNK_ROWS));
  p.waves = sp_copies(d, C);
  p.ld = SP_STAGE;
  p.lds = sp_lds_bytes(d, C, p.waves);   // with the exp table: the largest of the families
  return p;
}

hipError_t stk_launch_sweep_sparse(int family, const SweepLaunch& p, int shard0, int nsh, const SweepCall& c, hipStream_t st) {
  if (p.kind != SWEEP_SPARSE || !c.sp) return hipErrorInvalidValue;
  return sweep_family(family, [&](auto fam) -> hipError_t {
    constexpr int FAM = decltype(fam)::value;
    SweepArgs A{c.shards, c.q, c.partial, c.req_step, c.step_id, p.C, c.Dp, p.G, p.ld, sweep_pw(FAM, p.d), shard0, c.Gs, c.ran};
    A.Ct = c.Ct;
    A.c0 = c.c0;
    return stk_launch_sweep_sp<FAM>(p, A, c.sp, nsh * p.G, st);
  });
}
#endif  // STK_SWEEP_BASE

template <int FAM, int C>
static hipError_t go_sp(const SweepLaunch& p, const SweepArgs& A, const SpShardDev* sp, int nblocks, hipStream_t st) {
  auto kern = k_sweep_sp<FAM, C>;
  if (const hipError_t e = allow_big_lds((const void*)kern)) return e;
  hipLaunchKernelGGL(kern, dim3(nblocks), dim3(SP_NT), p.lds, st, A, sp);
  return hipGetLastError();
}

// Instantiated in the object that holds the family (STK_SWEEP_TU, sweep_common.h).
template <int FAM>
hipError_t stk_launch_sweep_sp(const SweepLaunch& p, const SweepArgs& A, const SpShardDev* sp, int nblocks, hipStream_t st) {
  if (!stk_sweep_sparse_supported(p.C, p.d) || p.waves != sp_copies(p.d, p.C) || p.ld != SP_STAGE ||
      p.lds != sp_lds_bytes(p.d, p.C, p.waves) || p.lds > BIG_LDS_BYTES)
    return hipErrorInvalidValue;
  switch (p.C) {
    case 1: return go_sp<FAM, 1>(p, A, sp, nblocks, st);
    case 2: return go_sp<FAM, 2>(p, A, sp, nblocks, st);
    case 4: return go_sp<FAM, 4>(p, A, sp, nblocks, st);
    case 8: return go_sp<FAM, 8>(p, A, sp, nblocks, st);
    case 16: return go_sp<FAM, 16>(p, A, sp, nblocks, st);
  }
  return hipErrorInvalidValue;
}
STK_SWEEP_INSTANTIATE(stk_launch_sweep_sp, const SweepLaunch&, const SweepArgs&, const SpShardDev*, int, hipStream_t)
