// The wide 16-chain regression sweep (C = 16, 128 < d <= 1024): a K-split of k_sweep16
// (sweep16.hip), whose per-wave slot of 16 rows x d columns stops fitting LDS past d = 128.
//
// Replaces the same gradient as k_sweep16 (the one Stan's autodiff computes inside `sm.sampling`,
// stark/stark.py:48; oracle: orc_logreg_lpgrad / orc_linreg_lpgrad).
//
// Workgroup = NW = ceil(d / 128) waves that SHARE every 16-row sub-tile of the block's chunk.  Wave w
// owns the column slab [w DW, w DW + DW), DW = 16 ceil(d / (16 NW)) <= 128 (the last slab may be
// partial), and a private LDS slot [16 rows][DW] for it, rows 16 B apart from a multiple of 128 B so
// the forward's ds_read_b128 (one row per lane of a group of 16) spread over the banks; every
// operand read is the lane's base address plus a compile-time offset.  Per sub-tile:
//   DMA       the wave's own slab, `buffer_load_dwordx4 ... lds` (nt: X is read once per sweep);
//             the LDS image is lane-linear, the per-lane SOURCE offset gathers the 16 row segments
//             (and repeats a row's last valid 16 B in the pad and past column d - 1); wave 0 also
//             loads the 16 y;
//   forward   a partial eta[16 rows][16 chains] over the slab on v_mfma_f64_16x16x4, beta of the
//             slab in registers for the whole launch, wave 0's accumulator starting at alpha;
//   exchange  the partials go to LDS; after one barrier every wave sums them in wave order
//             0 .. NW - 1, so every wave holds the same eta to the bit; a second barrier frees the
//             exchange area and y for the next sub-tile.  No DMA is in flight at either barrier
//             (the slab is waited for at the top of the sub-tile and reissued at its end), so
//             both are plain __syncthreads(): its vmcnt drain has nothing to wait for;
//   residual  logit_resid4 / the linear z / pois_resid on the summed eta, redundantly in every wave; wave 0's
//             lp terms and d/d alpha are the ones written out;
//   backward  G[slab columns][16 chains] += X_slab^T . d_eta from the wave's own slot, one MFMA per
//             (16-column tile, k-step); then the wave reissues its slab's DMA for the next sub-tile
//             (the slot is wave-private: only the exchange needs the barriers).
// A wave owns its columns over all the chunk's rows, so the chunk partial [chain][d + 2] is written
// straight from the accumulators: no block reduction.  Chunks depend on (n, d) only and every sum
// has a fixed order: the result is bitwise independent of the grid a shard is launched in.
//
// The library compiles this file once per STK_SWEEP_TU (sweep_common.h): the base object and one object per
// later family; a tool that includes it without the macro gets every family.
#include "sweep_common.h"
#include <math.h>
#include <algorithm>

namespace stk {

constexpr int SW_FLUSH = 32;    // sub-tiles between log1p flushes: 128 factors per lane, 1 + sp < 2^128
constexpr int SW_MAXW = 8;      // waves per block at most (d <= 1024)
constexpr int SW_TILES = 16;    // 64-row tiles per chunk at least
constexpr int SW_YB = 128;      // bytes of the y area (16 rows of 8 B)

__host__ __device__ constexpr int sw_waves(int d) { return (d + 127) / 128; }
__host__ __device__ constexpr int sw_slab(int d) { return 16 * ((d + 16 * sw_waves(d) - 1) / (16 * sw_waves(d))); }
__host__ __device__ constexpr int sw_row_bytes(int DW) { return DW * 8 + 16; }
__host__ __device__ constexpr int sw_slot_bytes(int DW) { return SM_R * sw_row_bytes(DW); }

// The DMAs go through plain functions (see dma16_lds in sweep.hip).
__device__ __forceinline__ void sw_dma16(__amdgpu_buffer_rsrc_t r, char* dst, int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_vptr)dst, 16, voff, soff, 0, 2);
}
__device__ __forceinline__ void sw_dma4(__amdgpu_buffer_rsrc_t r, char* dst, int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_vptr)dst, 4, voff, soff, 0, 2);
}

template <int FAM, int KF>
__global__ __launch_bounds__(64 * SW_MAXW) void k_sweep16w(SweepArgs A) {
  constexpr int C = SM_C, DW = 4 * KF, JT = KF / 4;
  constexpr int RSB = sw_row_bytes(DW), SLOTB = sw_slot_bytes(DW);
  constexpr int PPR = DW / 2 + 1;                   // 16-B pieces per padded row
  constexpr int NI = (SM_R * PPR + 63) / 64;        // DMA instructions per slot; the last one has 16 lanes
  constexpr bool LOGI = FAM == STK_LOGREG, NB = FAM == STK_NEGBIN, POIS = fam_yint(FAM) && !LOGI;   // POIS: whole int32 counts
  constexpr bool ST = FAM == STK_STUDENT;           // the linear layout (double y, 1 / sigma per chain), its own residual
  constexpr bool GM = FAM == STK_GAMMA;             // double ly = log y (fam_ydouble), the shape a per chain, the exp table
  static_assert(fam_known(FAM), "k_sweep16w: unknown family");
  constexpr int YB = fam_yint(FAM) ? 4 : 8;         // int32 y (logistic, poisson) or double y
  static_assert(KF % 4 == 0 && DW <= 128 && (SM_R * PPR) % 64 == 16, "slab geometry");
  const int NW = A.LD;                              // waves per block = column slabs
  const int shard = A.shard0 + blockIdx.x / A.G;
  const int chunk = blockIdx.x % A.G;
  if (A.req_step && A.req_step[shard] != A.step_id - 1) return;
  if (A.ran && chunk == 0 && threadIdx.x == 0) atomicAdd(&A.ran[A.step_id & 63], 1);
  const ShardDev sh = A.shards[shard];
  const int d = sh.d;
  const int tid = threadIdx.x, lane = tid & 63, w = uniform_int(tid >> 6);
  const int lr = lane & 15, lh = lane >> 4;
  const int64_t nt = (sh.n + 63) / 64;
  const int64_t t0 = nt * chunk / A.G, t1 = nt * (chunk + 1) / A.G;
  const int64_t r0 = t0 * 64, r1 = std::min<int64_t>(sh.n, t1 * 64);
  const int nrows = (int)(r1 - r0);
  const int nsub = (nrows + SM_R - 1) / SM_R;       // every wave takes every sub-tile
  const int j0 = w * DW;                            // first column of the wave's slab
  const int dwv = std::min(DW, d - j0);             // its columns below d (>= 1)

  extern __shared__ __attribute__((aligned(16))) double lds[];
  char* const slot = reinterpret_cast<char*>(lds) + (size_t)w * SLOTB;
  char* const ybuf = reinterpret_cast<char*>(lds) + (size_t)NW * SLOTB;
  double* const exch = reinterpret_cast<double*>(ybuf + SW_YB);   // [NW][4 registers][64 lanes]
  double* const tab = exch + (size_t)NW * 256;
  if constexpr (fam_exp_table(FAM)) exp_table_init(tab);
  const double* qs = A.q + chain_row(A, shard) * A.Dp;
  double bf[KF];                   // beta_{lr} at column j0 + lh KF + s (k-step s of lane group lh)
#pragma unroll
  for (int s = 0; s < KF; ++s) {
    const int col = j0 + lh * KF + s;
    bf[s] = col < d ? qs[(size_t)lr * A.Dp + 1 + col] : 0.0;
  }
  const double alpha = w == 0 ? qs[(size_t)lr * A.Dp] : 0.0;   // wave 0's partial starts at alpha
  // linear: 1 / sigma; negative binomial: v = log phi itself, with phi beside it (a lane is one chain)
  const double inv_s = fam_chain_scalar<FAM>(qs[(size_t)lr * A.Dp + d + 1]);
  double nbphi = 0.0;
  if constexpr (NB) nbphi = exp(inv_s);
  double nu = 0.0, nu1 = 0.0, inv_nu = 0.0;              // student_t: wave-uniform, read once
  if constexpr (ST) nu = shard_nu(sh), nu1 = nu + 1.0, inv_nu = 1.0 / nu;
  __syncthreads();
  __builtin_amdgcn_s_waitcnt(0xF70);

  const __amdgpu_buffer_rsrc_t xr = uniform_rsrc(sh.x + r0 * d, (int64_t)nrows * d * 8);
  const void* ybase = (LOGI || POIS) ? (const void*)(sh.yi + r0) : (const void*)(fam_ydouble<FAM>(sh) + r0);
  const __amdgpu_buffer_rsrc_t yr = uniform_rsrc(ybase, (int64_t)nrows * YB);
  // piece p = 64 j + lane of the slot image is piece p % PPR of row p / PPR; the pad piece and the
  // pieces past column d - 1 repeat the row's last valid piece (finite data under a zero beta)
  const int pmax = std::min(DW / 2 - 1, (dwv + 1) / 2 - 1);
  // LEAN (the negative binomial at the widest slab, whose residual leaves no room for them): the NI offsets
  // are recomputed at every issue instead of held in registers across the loop
  constexpr bool LEAN = NB && KF == 32;
  auto voff_at = [&](int j) {
    int ln = lane;
    if constexpr (LEAN) asm volatile("" : "+v"(ln));   // opaque: else the offsets are hoisted out of the loop again
    const int p = j * 64 + ln, row = std::min(p / PPR, SM_R - 1), pr = std::min(p % PPR, pmax);
    return row * d * 8 + pr * 16;
  };
  int voff[LEAN ? 1 : NI];
  if constexpr (!LEAN) {
#pragma unroll
    for (int j = 0; j < NI; ++j) voff[j] = voff_at(j);
  }
  auto issue = [&](int u) {           // 1 KiB per DMA instruction
    const int soff = u * SM_R * d * 8 + j0 * 8;
#pragma unroll
    for (int j = 0; j < NI - 1; ++j) sw_dma16(xr, slot + j * 1024, LEAN ? voff_at(j) : voff[j], soff);
    if (lane < 16) sw_dma16(xr, slot + (NI - 1) * 1024, LEAN ? voff_at(NI - 1) : voff[NI - 1], soff);
    if (w == 0 && lane < SM_R * YB / 4) sw_dma4(yr, ybuf, lane * 4, u * SM_R * YB);
  };

  dbl4 gacc[JT];
#pragma unroll
  for (int t = 0; t < JT; ++t) gacc[t] = dbl4{0.0, 0.0, 0.0, 0.0};
  double lm = 0.0, sp = 0.0, ll = 0.0, ga = 0.0;   // logistic lp pieces (linear: lm = sum z^2; poisson: lm = lp)
  const char* const xfw = slot + lr * RSB + lh * KF * 8;    // forward A: row lr, columns lh KF + s
  const char* const xbw = slot + lh * RSB + lr * 8;         // backward A: row lh + 4s, column 16t + lr

  if (nsub > 0) issue(0);
  for (int k = 0; k < nsub; ++k) {
    __builtin_amdgcn_s_waitcnt(0xF70);                 // vmcnt(0): the wave's slab of sub-tile k (and y) landed
    __builtin_amdgcn_sched_barrier(0);
    const int rv = std::min(SM_R, nrows - SM_R * k);
    // ---- forward over the slab: partial eta[row lh + 4i][chain lr]
    dbl4 ea0 = dbl4{alpha, alpha, alpha, alpha}, ea1 = dbl4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int m = 0; m < KF / 2; ++m) {
      const dbl2 x2 = *reinterpret_cast<const dbl2*>(xfw + m * 16);
      ea0 = mfma_f64(x2.x, bf[2 * m], ea0);
      ea1 = mfma_f64(x2.y, bf[2 * m + 1], ea1);
    }
    const dbl4 part = ea0 + ea1;
#pragma unroll
    for (int i = 0; i < 4; ++i) exch[(w * 4 + i) * 64 + lane] = part[i];
    __syncthreads();                                      // every wave's partial (and wave 0's y) is in LDS
    // ---- eta = the partials summed in wave order: the same bits in every wave
    dbl4 eta4;
#pragma unroll
    for (int i = 0; i < 4; ++i) eta4[i] = exch[i * 64 + lane];
    for (int ww = 1; ww < NW; ++ww)
#pragma unroll
      for (int i = 0; i < 4; ++i) eta4[i] += exch[(ww * 4 + i) * 64 + lane];
    uint32_t ym[4];
    double yv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (LOGI || POIS)   // int32 y: {0, 1} (logistic), the whole count (poisson)
        ym[i] = *reinterpret_cast<const uint32_t*>(ybuf + (lh + 4 * i) * 4);
      else
        yv[i] = *reinterpret_cast<const double*>(ybuf + (lh + 4 * i) * 8);
    }
    __syncthreads();                                      // the exchange area and y are free for sub-tile k + 1

    // ---- residual (as k_sweep16)
    double de[4];
    if (rv == SM_R) {                                  // full sub-tile: no masks
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if constexpr (LOGI) {
          de[i] = logit_resid4(eta4[i], ym[i], tab, lm, sp);
        } else if constexpr (NB) {
          de[i] = negbin_resid(eta4[i], (int32_t)ym[i], inv_s, nbphi, tab, lm, sp);
          __builtin_amdgcn_sched_barrier(0);   // one element's temporaries at a time: interleaved, the four spill
        } else if constexpr (ST) {
          de[i] = student_resid(eta4[i], yv[i], inv_s, nu, nu1, inv_nu, lm, sp);
        } else if constexpr (GM) {
          de[i] = gamma_resid(eta4[i], yv[i], inv_s, tab, lm);
        } else if constexpr (POIS) {
          de[i] = pois_resid(eta4[i], (int32_t)ym[i], tab, lm);
        } else {
          const double z = (yv[i] - eta4[i]) * inv_s;
          lm = fma(z, z, lm);
          de[i] = z * inv_s;
        }
        ga += de[i];
      }
    } else {                                           // a chunk's last sub-tile
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool valid = lh + 4 * i < rv;
        double lm2 = lm, sp2 = sp, dv;
        if constexpr (LOGI) {
          dv = logit_resid4(eta4[i], ym[i], tab, lm2, sp2);
        } else if constexpr (NB) {
          dv = negbin_resid(eta4[i], (int32_t)ym[i], inv_s, nbphi, tab, lm2, sp2);
          __builtin_amdgcn_sched_barrier(0);
        } else if constexpr (ST) {
          dv = student_resid(eta4[i], yv[i], inv_s, nu, nu1, inv_nu, lm2, sp2);
        } else if constexpr (GM) {
          dv = gamma_resid(eta4[i], yv[i], inv_s, tab, lm2);
        } else if constexpr (POIS) {
          dv = pois_resid(eta4[i], (int32_t)ym[i], tab, lm2);
        } else {
          const double z = (yv[i] - eta4[i]) * inv_s;
          lm2 = fma(z, z, lm);
          dv = z * inv_s;
        }
        lm = valid ? lm2 : lm;
        sp = valid ? sp2 : sp;
        de[i] = valid ? dv : 0.0;
        ga += de[i];
      }
    }
    // ---- backward over the slab
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int t = 0; t < JT; ++t)
        gacc[t] = mfma_f64(*reinterpret_cast<const double*>(xbw + s * 4 * RSB + t * 128), de[s], gacc[t]);
    __builtin_amdgcn_s_waitcnt(0xC07F);                // lgkmcnt(0): the slot is free
    __builtin_amdgcn_sched_barrier(0);
    if (k + 1 < nsub) issue(k + 1);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (LOGI) {
      if ((k % SW_FLUSH) == SW_FLUSH - 1) {
        ll += log1p(sp);
        sp = 0.0;
      }
    }
  }
  double lpa;
  if constexpr (LOGI) {   // the residual returned -dv: negate the gradient sums once
    lpa = 0.5 * lm - (ll + log1p(sp));
    ga = -ga;
#pragma unroll
    for (int t = 0; t < JT; ++t) gacc[t] = -gacc[t];
  } else {   // linear: sum z^2, finished in the reduce; poisson: lp itself (pois_resid returns dv)
    lpa = lm;
  }

  // ---- the chunk's partial row per chain: the wave's own columns; lp and d/d alpha from wave 0,
  // its four lane groups (rows lh + 4i) added as (0 + 1) + (2 + 3)
  double* out = A.partial + ((size_t)shard * A.Gs + chunk) * C * A.PW + (size_t)lr * A.PW;
#pragma unroll
  for (int t = 0; t < JT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = j0 + 16 * t + lh + 4 * i;
      if (j < d) out[1 + j] = gacc[t][i];
    }
  if (w == 0) {
    lpa += __shfl_xor(lpa, 16);
    ga += __shfl_xor(ga, 16);
    lpa += __shfl_xor(lpa, 32);
    ga += __shfl_xor(ga, 32);
    if (lh == 0) {
      out[d + 1] = lpa;
      out[0] = ga;
    }
    if constexpr (fam_sum3(FAM)) {   // the third scalar sum (sp holds sum sp(t); student_t: sum z^2 / (nu + z^2)), column d + 2, joined the same way
      sp += __shfl_xor(sp, 16);
      sp += __shfl_xor(sp, 32);
      if (lh == 0) out[d + 2] = sp;
    }
  }
}

}  // namespace stk

#include "launchers.h"
using namespace stk;

#ifdef STK_SWEEP_BASE
bool stk_sweep16w_supported(int d) { return d > 128 && d <= 128 * SW_MAXW; }
int stk_sweep16w_waves(int d) { return sw_waves(d); }
int stk_sweep16w_chunks(int64_t n) {                  // >= SW_TILES tiles of 64 rows per chunk
  const int64_t nt = (n + 63) / 64;
  return (int)std::max<int64_t>(1, std::min<int64_t>(512, (nt + SW_TILES - 1) / SW_TILES));
}
size_t stk_sweep16w_lds_bytes(int family, int d) {
  const int nw = sw_waves(d);
  return (size_t)nw * sw_slot_bytes(sw_slab(d)) + SW_YB + (size_t)nw * 256 * 8 + (fam_exp_table(family) ? EX_TAB * 8 : 0);
}
#endif

template <int FAM, int KF>
static hipError_t go16w(const SweepArgs& A, int nblocks, size_t lds, hipStream_t st) {
  auto kern = k_sweep16w<FAM, KF>;
  if (const hipError_t e = allow_big_lds((const void*)kern)) return e;
  hipLaunchKernelGGL(kern, dim3(nblocks), dim3(64 * A.LD), lds, st, A);
  return hipGetLastError();
}

// Instantiated in the object that holds the family (STK_SWEEP_TU, sweep_common.h).
template <int FAM>
hipError_t stk_launch_sweep16w(const SweepArgs& A, int d, int nblocks, size_t lds, hipStream_t st) {
  if (!stk_sweep16w_supported(d) || A.LD != sw_waves(d) || lds < stk_sweep16w_lds_bytes(FAM, d) || lds > BIG_LDS_BYTES)
    return hipErrorInvalidValue;
  switch (sw_slab(d) / 4) {
    case 20: return go16w<FAM, 20>(A, nblocks, lds, st);
    case 24: return go16w<FAM, 24>(A, nblocks, lds, st);
    case 28: return go16w<FAM, 28>(A, nblocks, lds, st);
    case 32: return go16w<FAM, 32>(A, nblocks, lds, st);
  }
  return hipErrorInvalidValue;
}
STK_SWEEP_INSTANTIATE(stk_launch_sweep16w, const SweepArgs&, int, int, size_t, hipStream_t)
