// The weighted-likelihood bootstrap sweep (regression families, 1 <= d <= 128): log density + gradient of
// 16 bootstrap replicates of a shard in ONE pass over the shard's rows, on the fp64 MFMA.  Row i of
// replicate b carries the random weight w_ib of boot_math.h -- Exp(1) for the weighted-likelihood
// ("Bayesian") bootstrap of Newton and Raftery, Poisson(1) for the classical bootstrap in the form that
// shards -- made in the kernel from Philox: a pure function of (seed, stream, row, replicate), never
// stored.  No reference counterpart (its README names the mode as future work); engine.bootstrap turns
// the sweep into B replicates of the full-data maximiser.
//
//   lp_b   = sum_i w_ib ll_i(q_b) + prior(q_b) + Jacobian        ll_i, prior, Jacobian: k_sweep_reduce's
//   grad_b = its gradient [D]                                    (sweep.hip), linear's -n u becomes -wsum_b u
//   wsum_b = sum_i w_ib
//
// k_boot16 is the weighted twin of k_sweep16 (sweep16.hip) and keeps its shape: 4 waves per workgroup and
// two workgroups per CU, wave w owns the 16-row sub-tiles u = w, w + 4, ... of its chunk, the sub-tile's
// rows and y arrive in the wave's LDS slot by `buffer_load_dwordx4 ... lds`, eta[16 rows][16 replicates]
// = alpha_b + x_i . beta_b on v_mfma_f64_16x16x4 with beta in registers, the residual on the MFMA output
// registers, the backward X^T (w . d_eta) on the MFMA again (a last tile of <= 4 columns on the VALU by
// DPP).  What differs:
//   chunks    G = boot_chunks(n) depends on n alone, and a chunk starts at a multiple of 64 rows: every
//             sub-tile starts at a multiple of 16, which is what lets ONE Philox call per lane and
//             sub-tile give the lane the weights of its four rows lh, lh + 4, lh + 8, lh + 12;
//   weights   made before the wait for the sub-tile's DMA (they need the row index only);
//   residual  every row has its own weight, so the sampler's running product of (1 + e) does not apply:
//             logistic ll = min(t, 0) - log1p(e), e = exp(-|eta|), t = (2 y - 1) eta, through
//             predictive_math.h's pd_exp / pd_log1p01 / pd_rcp (about 2 ulp each, branch-free); poisson
//             ll = y eta - exp(eta) (pd_exp, a NaN eta put back); linear sum w z^2, finished in the reduce.
//             Rows past the shard's end get weight 0 by select: what a padding row computes is dropped.
// Chunk partials [16][d + 3] (alpha, beta, the lp sum, wsum) are summed in chunk order by k_boot_reduce.
// An MFMA output column depends on its own B column only and every sum runs in an order fixed by (n, d),
// so a replicate's three outputs depend on (shard rows, seed, stream, b, q_b) alone, bit for bit: not on
// its companions in the call, on R, on how many shards share the launch or on the device.
#include "sweep_common.h"
#include "predictive_math.h"
#include "boot_math.h"
#include "launchers.h"
#include <math.h>
#include <algorithm>

namespace stk {

constexpr int BT_GPC = 4;          // 64-row groups per chunk before the chunk count saturates
constexpr int BT_GMAX = 512;       // chunks per shard at most: one round of two workgroups per CU

__host__ __device__ inline int boot_chunks(int64_t n) {
  const int64_t ng = (n + 63) / 64, g = (ng + BT_GPC - 1) / BT_GPC;
  return (int)(g < 1 ? 1 : (g > BT_GMAX ? BT_GMAX : g));
}
// rows of the longest chunk: the buffer descriptor of a chunk holds its bytes in 31 bits
__host__ __device__ inline int64_t boot_chunk_rows(int64_t n) {
  const int64_t nt = (n + 63) / 64, G = boot_chunks(n);
  return 64 * ((nt + G - 1) / G);
}

// Column tiles of the backward pass at KF = ceil(d / 4) k-steps (k_sweep16's geometry).
struct BootGeom {
  int KF, JT, REM, JTM;
  bool VREM;
};
__host__ __device__ constexpr BootGeom boot_geom(int KF) {
  const int JT = (KF + 3) / 4;                  // 16-column tiles covering 4 KF >= d columns
  const int REM = 4 * KF - 16 * (JT - 1);       // columns of the last tile (d has up to 3 fewer)
  const bool VREM = REM <= 4;                   // <= 4: the VALU does the last tile
  return BootGeom{KF, JT, REM, VREM ? JT - 1 : JT, VREM};
}
// Early release of the slot (the backward's A operands move to registers after the forward, and the next
// sub-tile's DMA starts before the residual): k_sweep16's rule.  Through KF = 27 (d <= 108) every family
// stays within 256 VGPRs without scratch (logistic: 254 at KF = 27); past that the slot is released
// after the backward.
__host__ __device__ constexpr bool boot_pre(int KF) { return KF <= 27; }

__host__ __device__ constexpr size_t boot_lds_bytes_kf(int d, int KF) {
  const size_t main = (size_t)SM_W * sweepm_slot_bytes(d) + EX_TAB * 8;
  const size_t red = ((size_t)SM_W * boot_geom(KF).JT * 16 * 16 + (size_t)SM_W * 64 * 3 + (size_t)SM_W * 4 * 4 * 16) * 8;
  return main > red ? main : red;
}

struct BootArgs {
  const ShardDev* shards;
  const double* q;          // [16][Dp] the tile's points (the last one repeated to fill)
  double* partial;          // [nsh][Gs][16][PW] chunk partials
  const int32_t* streams;   // [nsh] the stream of every shard of the launch
  double* lp;               // [nsh][R]
  double* grad;             // [nsh][R][D]
  double* wsum;             // [nsh][R]
  uint64_t seed;
  int shard0, Gs, Dp, PW;
  int rep0;                 // replicate index of the tile's column 0 (a multiple of 16)
  int kind;
  int R, c0, nrep;          // replicates of the call, the tile's first row in lp / grad / wsum, its live columns
};

template <int FAM, int KF, bool PRE = boot_pre(KF), int NACC = 2>
__global__ __launch_bounds__(256, 2) void k_boot16(BootArgs A) {
  constexpr BootGeom g = boot_geom(KF);
  constexpr int C = SM_C, NW = SM_W, JTM = g.JTM;
  constexpr bool LOGI = FAM == STK_LOGREG, POIS = FAM == STK_POISSON;
  static_assert(LOGI || POIS || FAM == STK_LINREG, "k_boot16: unknown family");
  const int si = blockIdx.y, chunk = blockIdx.x;
  const ShardDev sh = A.shards[A.shard0 + si];
  const int G = boot_chunks(sh.n);
  if (chunk >= G) return;                            // block-uniform
  const int d = sh.d;
  const int tid = threadIdx.x, lane = tid & 63, w = uniform_int(tid >> 6);
  const int lr = lane & 15, lh = lane >> 4;
  const int64_t nt = (sh.n + 63) / 64;
  const int64_t t0 = nt * chunk / G, t1 = nt * (chunk + 1) / G;
  const int64_t r0 = t0 * 64, r1 = std::min<int64_t>(sh.n, t1 * 64);
  const int nrows = (int)(r1 - r0);
  const int nsub = (nrows + SM_R - 1) / SM_R;
  const int mine = nsub > w ? (nsub - w + NW - 1) / NW : 0;   // own sub-tiles u = w + NW k
  constexpr int YB = (LOGI || POIS) ? 4 : 8;       // int32 y (logistic, poisson) or double y
  const int SBX = SM_R * d * 8;
  const int SS = sweepm_slot_bytes(d);

  extern __shared__ __attribute__((aligned(16))) double lds[];
  char* const slot = reinterpret_cast<char*>(lds) + (size_t)w * SS;
  double* const tab = reinterpret_cast<double*>(reinterpret_cast<char*>(lds) + (size_t)NW * SS);
  if constexpr (LOGI || POIS) exp_table_init(tab);
  const double* qs = A.q;
  double bf[KF];                   // beta_{lr} at the column k-step s of lane group lh takes (forward)
#pragma unroll
  for (int s = 0; s < KF; ++s) {
    const int col = (d & 1) ? lh * KF + s : (s < KF - (KF & 1) ? 8 * (s / 2) + 2 * lh + (s & 1) : 8 * (KF / 2) + lh);
    bf[s] = col < d ? qs[(size_t)lr * A.Dp + 1 + col] : 0.0;
  }
  const double alpha = qs[(size_t)lr * A.Dp];
  const double inv_s = FAM == STK_LINREG ? exp(-qs[(size_t)lr * A.Dp + d + 1]) : 0.0;
  const uint32_t stream = (uint32_t)A.streams[si], rep = (uint32_t)(A.rep0 + lr);
  __syncthreads();
  __builtin_amdgcn_s_waitcnt(0xF70);

  const __amdgpu_buffer_rsrc_t xr = uniform_rsrc(sh.x + r0 * d, (int64_t)nrows * d * 8);
  const void* ybase = (LOGI || POIS) ? (const void*)(sh.yi + r0) : (const void*)(sh.y + r0);
  const __amdgpu_buffer_rsrc_t yr = uniform_rsrc(ybase, (int64_t)nrows * YB);
  const int nx = (SBX + 1023) >> 10;
  const int last_lanes = (SBX - ((nx - 1) << 10)) >> 4;
  auto issue = [&](int k) {           // 1 KiB per DMA instruction, aux = 2 (nt); past the chunk's bytes: zeros
    const int u = w + NW * k;
    const int xoff = u * SBX;
    for (int j = 0; j < nx - 1; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_vptr)(slot + j * 1024), 16, lane * 16, xoff + j * 1024, 0, 2);
    if (lane < last_lanes)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_vptr)(slot + (nx - 1) * 1024), 16, lane * 16,
                                               xoff + (nx - 1) * 1024, 0, 2);
    if (lane < SM_R * YB / 4)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(yr, (lds_vptr)(slot + SBX), 4, lane * 4, u * SM_R * YB, 0, 2);
  };

  dbl4 gacc[JTM > 0 ? JTM : 1];
#pragma unroll
  for (int t = 0; t < JTM; ++t) gacc[t] = dbl4{0.0, 0.0, 0.0, 0.0};
  double gv[4] = {0.0, 0.0, 0.0, 0.0};
  double lm = 0.0, ga = 0.0, ws = 0.0;             // sum w ll (linear: sum w z^2), sum d_eta, sum w
  const double* xs = reinterpret_cast<const double*>(slot);
  // column of the backward's A operand in tile t: only a last MFMA tile (no VALU remainder) can reach
  // past d - 1, so only it is clamped
  auto bcol = [&](int t) { return (g.VREM || t < JTM - 1) ? 16 * t + lr : std::min(16 * t + lr, d - 1); };
  const double* xrow = xs + lr * d;

  if (mine > 0) issue(0);
  for (int k = 0; k < mine; ++k) {
    // ---- the weights of rows lh + 4 i of replicate lr: one Philox call, while the DMA is in flight
    const int64_t row0 = r0 + (int64_t)SM_R * (w + NW * k);   // a multiple of 16
    uint32_t wd[4];
    boot_words(A.seed, stream, row0 + lh, rep, wd);
    double wt[4];
    if (A.kind == BOOT_POISSON) {
#pragma unroll
      for (int i = 0; i < 4; ++i) wt[i] = (double)boot_poisson(wd[i]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) wt[i] = boot_exponential(wd[i]);
    }
    __builtin_amdgcn_s_waitcnt(0xF70);                 // vmcnt(0): sub-tile k landed
    __builtin_amdgcn_sched_barrier(0);
    const int rv = std::min(SM_R, nrows - SM_R * (w + NW * k));
    // ---- forward: eta[row lh + 4i][replicate lr], starting from alpha
    dbl4 ea[NACC];
    ea[0] = dbl4{alpha, alpha, alpha, alpha};
#pragma unroll
    for (int i = 1; i < NACC; ++i) ea[i] = dbl4{0.0, 0.0, 0.0, 0.0};
    if ((d & 1) == 0) {
      // even d (16-B aligned rows): k-steps 2m, 2m + 1 of lane group lh take columns 8m + 2 lh and
      // 8m + 2 lh + 1 (one 16-byte LDS read per pair); KF odd: the last k-step takes column 8 (KF / 2) + lh.
      // Odd d: k-step s of lane group lh takes column lh KF + s
#pragma unroll
      for (int m = 0; m < KF / 2; ++m) {
        const dbl2 x2 = *reinterpret_cast<const dbl2*>(xs + lr * d + 8 * m + 2 * lh);
        ea[(2 * m) % NACC] = mfma_f64(x2.x, bf[2 * m], ea[(2 * m) % NACC]);
        ea[(2 * m + 1) % NACC] = mfma_f64(x2.y, bf[2 * m + 1], ea[(2 * m + 1) % NACC]);
      }
      if constexpr (KF & 1) {
        const int col = 8 * (KF / 2) + lh;
        ea[(KF - 1) % NACC] = mfma_f64(xrow[std::min(col, d - 1)], bf[KF - 1], ea[(KF - 1) % NACC]);
      }
    } else {
#pragma unroll
      for (int s = 0; s < KF; ++s) {
        // lh KF + s <= d - 1 unless s >= KF - 3 (d >= 4 KF - 3): clamp those steps only
        ea[s % NACC] = mfma_f64(xrow[s < KF - 3 ? lh * KF + s : std::min(lh * KF + s, d - 1)], bf[s], ea[s % NACC]);
      }
    }
    // ---- everything else the sub-tile needs from the slot, into registers; then release it
    double xa[4][PRE && JTM > 0 ? JTM : 1];
    if constexpr (PRE) {
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int t = 0; t < JTM; ++t) xa[s][t] = xs[(lh + 4 * s) * d + bcol(t)];
    }
    // the VALU last tile's X: ONE value per lane, row lh + 4 (lr >> 2), column 16 JTM + (lr & 3) --
    // the value of (row lh + 4i, column jj) is then lane 4i + jj of the lane's own DPP row
    double xv = 0.0;
    if constexpr (g.VREM) xv = xs[(lh + 4 * (lr >> 2)) * d + std::min(16 * JTM + (lr & 3), d - 1)];
    uint32_t ym[4];
    double yv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (LOGI || POIS)   // int32 y: {0, 1} (logistic), the whole count (poisson)
        ym[i] = *reinterpret_cast<const uint32_t*>(slot + SBX + (lh + 4 * i) * 4);
      else
        yv[i] = *reinterpret_cast<const double*>(slot + SBX + (lh + 4 * i) * 8);
    }
    if constexpr (PRE) {
      __builtin_amdgcn_s_waitcnt(0xC07F);              // lgkmcnt(0): the slot is free
      __builtin_amdgcn_sched_barrier(0);
      if (k + 1 < mine) issue(k + 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    dbl4 eta4 = ea[0];
#pragma unroll
    for (int i = 1; i < NACC; ++i) eta4 += ea[i];

    // ---- weighted residual: lm += w ll, d_eta = w dll/deta; a row past the end is dropped by select
    double de[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool valid = lh + 4 * i < rv;
      const double eta = eta4[i];
      double term, dv;
      if constexpr (LOGI) {
        const bool y1 = ym[i] != 0u;
        const double t = y1 ? eta : -eta;
        const double e = pd_exp(-fabs(eta), tab);      // a NaN eta gives 0 here and stays NaN in t
        const double ri = pd_rcp(1.0 + e);
        term = 0.5 * (t - fabs(t)) - pd_log1p01(e);
        const double fr = t < 0.0 ? ri : e * ri;       // sigmoid(-t)
        dv = (y1 ? fr : -fr) + (eta - eta);            // + 0, or the NaN of a non-finite eta
      } else if constexpr (POIS) {
        const double yd = (double)(int32_t)ym[i];
        double mu = pd_exp(eta, tab);
        mu = eta != eta ? eta : mu;                    // pd_exp turns a NaN into 0: put it back
        term = fma(yd, eta, -mu);
        dv = yd - mu;
      } else {
        const double z = (yv[i] - eta) * inv_s;
        term = z * z;
        dv = z * inv_s;
      }
      const double lm2 = fma(wt[i], term, lm);
      lm = valid ? lm2 : lm;
      de[i] = valid ? wt[i] * dv : 0.0;
      ws += valid ? wt[i] : 0.0;
      ga += de[i];
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- backward
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int t = 0; t < JTM; ++t)
        gacc[t] = mfma_f64(PRE ? xa[s][t] : xs[(lh + 4 * s) * d + bcol(t)], de[s], gacc[t]);
    if constexpr (g.VREM) {
      // gv[jj] += X[lh + 4i][16 JTM + jj] * de[i] with the X value broadcast from lane 4i + jj of the
      // row by v_fmac_f64_dpp row_newbcast (k_sweep16's remainder tile).  s_nop 1: the two wait states
      // a VALU write of the DPP source needs before the DPP read, should the register allocator copy xv
#define BT_DPP_FMAC(I, J, G) "v_fmac_f64_dpp %" #G ", %4, %" #I " row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"
      asm volatile("s_nop 1\n\t"
                   BT_DPP_FMAC(5, 0, 0) BT_DPP_FMAC(5, 1, 1) BT_DPP_FMAC(5, 2, 2) BT_DPP_FMAC(5, 3, 3)
                   BT_DPP_FMAC(6, 4, 0) BT_DPP_FMAC(6, 5, 1) BT_DPP_FMAC(6, 6, 2) BT_DPP_FMAC(6, 7, 3)
                   BT_DPP_FMAC(7, 8, 0) BT_DPP_FMAC(7, 9, 1) BT_DPP_FMAC(7, 10, 2) BT_DPP_FMAC(7, 11, 3)
                   BT_DPP_FMAC(8, 12, 0) BT_DPP_FMAC(8, 13, 1) BT_DPP_FMAC(8, 14, 2) BT_DPP_FMAC(8, 15, 3)
                   : "+v"(gv[0]), "+v"(gv[1]), "+v"(gv[2]), "+v"(gv[3])
                   : "v"(xv), "v"(de[0]), "v"(de[1]), "v"(de[2]), "v"(de[3]));
#undef BT_DPP_FMAC
    }
    if constexpr (!PRE) {
      __builtin_amdgcn_s_waitcnt(0xC07F);              // lgkmcnt(0): the slot is free
      __builtin_amdgcn_sched_barrier(0);
      if (k + 1 < mine) issue(k + 1);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- fixed-order block reduction -> one partial row per replicate
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __syncthreads();
  double* red = lds;                                   // [NW][JT*16 columns][16 replicates]
  constexpr int JC = g.JT * 16;
#pragma unroll
  for (int t = 0; t < JTM; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) red[((size_t)w * JC + 16 * t + lh + 4 * i) * 16 + lr] = gacc[t][i];
  double* red2 = red + (size_t)NW * JC * 16;           // [NW][64 lanes][lp, g_alpha, wsum]
  red2[(size_t)tid * 3 + 0] = lm;
  red2[(size_t)tid * 3 + 1] = ga;
  red2[(size_t)tid * 3 + 2] = ws;
  double* red3 = red2 + (size_t)NW * 64 * 3;           // VREM: [NW][4 lh][4 jj][16 replicates]
  if constexpr (g.VREM) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) red3[((size_t)(w * 4 + lh) * 4 + jj) * 16 + lr] = gv[jj];
  }
  __syncthreads();
  double* out = A.partial + ((size_t)si * A.Gs + chunk) * C * A.PW;
  const int jv = 16 * JTM;                             // first column summed from red3
  for (int i = tid; i < C * d; i += NW * 64) {
    const int c = i / d, j = i % d;
    double v = 0.0;
    if (j < jv) {
      for (int ww = 0; ww < NW; ++ww) v += red[((size_t)ww * JC + j) * 16 + c];
    } else {
      for (int ww = 0; ww < NW; ++ww)
        for (int h = 0; h < 4; ++h) v += red3[((size_t)(ww * 4 + h) * 4 + (j - jv)) * 16 + c];
    }
    out[(size_t)c * A.PW + 1 + j] = v;
  }
  if (tid < 3 * C) {          // replicate c: lanes h*16 + c of every wave, in (wave, h) order
    const int c = tid / 3, what = tid % 3;
    double v = 0.0;
    for (int ww = 0; ww < NW; ++ww)
      for (int h = 0; h < 4; ++h) v += red2[(size_t)(ww * 64 + h * 16 + c) * 3 + what];
    out[(size_t)c * A.PW + (what == 0 ? d + 1 : (what == 1 ? 0 : d + 2))] = v;
  }
}

// The chunk partials of every (shard, live replicate, column) of the tile summed in chunk order, then the
// family's closing terms, the normal(0, s) priors (unweighted) and the Jacobian of sigma = e^u
// (k_sweep_reduce's formulas with n replaced by wsum).
__global__ __launch_bounds__(256) void k_boot_reduce(BootArgs A, int family) {
  const int si = blockIdx.y;
  const ShardDev sh = A.shards[A.shard0 + si];
  const int d = sh.d, D = sh.D, G = boot_chunks(sh.n), PW = A.PW;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= A.nrep * PW) return;
  const int c = idx / PW, o = idx - c * PW;
  const size_t stride = (size_t)SM_C * PW;
  const double* src = A.partial + ((size_t)si * A.Gs * SM_C + c) * PW;
  double t = src[o];
  for (int k = 1; k < G; ++k) t += src[(size_t)k * stride + o];
  const size_t row = (size_t)si * A.R + A.c0 + c;
  if (o == d + 2) {
    A.wsum[row] = t;
    return;
  }
  const double* qc = A.q + (size_t)c * A.Dp;
  double* g = A.grad + row * D;
  double prior_g = 0.0, prior_lp = 0.0;
  if (sh.pa != 0.0 || sh.pb != 0.0) {
    if (o == 0) prior_g = -sh.pa * qc[0];
    else if (o <= d) prior_g = -sh.pb * qc[o];
    else {
      double sb = 0.0;
      for (int j = 1; j <= d; ++j) sb = fma(qc[j], qc[j], sb);
      prior_lp = -0.5 * (sh.pa * qc[0] * qc[0] + sh.pb * sb);
    }
  }
  if (family != STK_LINREG) {                        // the sums are lp and the gradient themselves
    if (o == d + 1) A.lp[row] = t + prior_lp;
    else g[o] = t + prior_g;
  } else if (o == d + 1) {                           // linear: sigma = exp(u) and its Jacobian
    double wsum = src[d + 2];
    for (int k = 1; k < G; ++k) wsum += src[(size_t)k * stride + d + 2];
    const double u = qc[d + 1];
    g[d + 1] = -wsum + t + 1.0;
    A.lp[row] = -0.5 * t - wsum * u + u + prior_lp;
  } else {
    g[o] = t + prior_g;
  }
}

template <int FAM, int KF>
static hipError_t go_boot(const BootArgs& A, int d, int nsh, hipStream_t st) {
  auto kern = k_boot16<FAM, KF>;
  if (const hipError_t e = allow_big_lds((const void*)kern)) return e;
  hipLaunchKernelGGL(kern, dim3(A.Gs, nsh), dim3(SM_W * 64), boot_lds_bytes_kf(d, KF), st, A);
  return hipGetLastError();
}

template <int FAM>
static hipError_t launch_boot(const BootArgs& A, int d, int nsh, hipStream_t st) {
  switch ((d + 3) / 4) {
#define BT_CASE(K) case K: return go_boot<FAM, K>(A, d, nsh, st);
    BT_CASE(1) BT_CASE(2) BT_CASE(3) BT_CASE(4) BT_CASE(5) BT_CASE(6) BT_CASE(7) BT_CASE(8)
    BT_CASE(9) BT_CASE(10) BT_CASE(11) BT_CASE(12) BT_CASE(13) BT_CASE(14) BT_CASE(15) BT_CASE(16)
    BT_CASE(17) BT_CASE(18) BT_CASE(19) BT_CASE(20) BT_CASE(21) BT_CASE(22) BT_CASE(23) BT_CASE(24)
    BT_CASE(25) BT_CASE(26) BT_CASE(27) BT_CASE(28) BT_CASE(29) BT_CASE(30) BT_CASE(31) BT_CASE(32)
#undef BT_CASE
  }
  return hipErrorInvalidValue;
}

}  // namespace stk

using namespace stk;

bool stk_boot_supported(int d) { return d >= 1 && d <= 128; }
int stk_boot_chunks(int64_t n) { return boot_chunks(n); }
int64_t stk_boot_chunk_rows(int64_t n) { return boot_chunk_rows(n); }
int stk_boot_rows_per_tile() { return SM_R; }
int stk_boot_waves() { return SM_W; }
size_t stk_boot_lds_bytes(int d) { return boot_lds_bytes_kf(d, (d + 3) / 4); }
// chunk-partial workspace of one shard for one tile of 16 replicates
size_t stk_boot_ws_bytes(int64_t n, int d) { return sizeof(double) * SM_C * (size_t)(d + 3) * boot_chunks(n); }

// One tile of 16 replicates (nrep live, the tile's points at q [16][Dp], replicate indices rep0 ..) against
// shards [shard0, shard0 + nsh): rows c0 .. c0 + nrep - 1 of lp [nsh][R], grad [nsh][R][D], wsum [nsh][R].
// partial holds nsh * Gs chunk blocks of 16 (d + 3) doubles, Gs >= every shard's chunk count; streams (device)
// one value per shard of the launch.  One sweep launch and one reduce launch.
hipError_t stk_launch_boot(int family, const ShardDev* shards, int shard0, int nsh, int d, int Gs, int Dp,
                           const double* q, double* partial, const int32_t* streams, uint64_t seed, int rep0, int kind,
                           int R, int c0, int nrep, double* lp, double* grad, double* wsum, hipStream_t st) {
  const BootArgs A{shards, q, partial, streams, lp, grad, wsum, seed, shard0, Gs, Dp, d + 3, rep0, kind, R, c0, nrep};
  hipError_t e = hipErrorInvalidValue;
  if (family == STK_LOGREG) e = launch_boot<STK_LOGREG>(A, d, nsh, st);
  else if (family == STK_LINREG) e = launch_boot<STK_LINREG>(A, d, nsh, st);
  else if (family == STK_POISSON) e = launch_boot<STK_POISSON>(A, d, nsh, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_boot_reduce, dim3((unsigned)((nrep * (d + 3) + 255) / 256), nsh), dim3(256), 0, st, A, family);
  return hipGetLastError();
}
