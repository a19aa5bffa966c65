// The softmax-regression sweep (STK_CATEGORICAL, include/stark_hip.h): log density + gradient of up to 16 chains of
// a shard in ONE pass over the shard's rows on the fp64 MFMA, K = ncat classes, G = K - 1 linear predictors per row.
//
//   y[n] ~ categorical_logit(append_row(alpha + x[n] * beta, 0))          class K is the reference, eta = 0
//   q = [alpha_1 .. alpha_G, beta_1[0 .. d), ..., beta_G[0 .. d)]          D = G (d + 1), Stan's own order
//
// k_sweep16's skeleton (sweep16.hip): 4 waves, the shard cut into chunks that depend on (n, d) alone, wave w owns the
// 16-row sub-tiles u = w, w + 4, ... of its chunk, `buffer_load ... lds` DMA of 16 rows of X and their int32 y into
// the wave's slot, fixed-order block reduction, chunk partials summed in chunk order by k_sweep_reduce_cat below.
// Chains lie along the MFMA's 16 columns and classes along accumulator tiles:
//   forward   eta_g[16 rows][16 chains], g < G: per k-step ONE A operand (a column of X, lane group lh = lane >> 4
//             takes column 4 s + lh of row lane & 15) feeds G v_mfma_f64_16x16x4, the B operand beta_g of chain
//             lane & 15 from the block's beta image in LDS; alpha_g is added to the accumulators afterwards.  A lane then holds
//             eta of rows lh + 4 i, chain lane & 15, ALL G classes in its own registers;
//   residual  within the lane, no cross-lane traffic: m = max(0, max_g eta_g), G + 1 table exponentials
//             e_g = exp(eta_g - m), e_0 = exp(-m), s = e_0 + sum_g e_g in [1, K], one reciprocal,
//               lp      += eta_y - m - log s           (eta_K = 0)
//               d eta_g  = 1[y = g] - e_g / s
//             log s is not taken per element: the lane keeps the running product of s and, after every sub-tile (four
//             factors of at most 17), moves its exponent into an integer by v_frexp -- exact, so the product never
//             overflows and each factor adds at most one ulp of relative error; one log per lane at the end;
//   backward  gacc[g][t] += X_tile^T . d eta_g for class g and 16-column tile t, four MFMAs each: the D layout of the
//             forward is the B layout of the backward, as in k_sweep16; one A operand serves the G classes.  The last
//             tile's columns past d - 1 are clamped to d - 1 and their sums never written.
// beta is a block image in LDS ([G][16 JT columns][16 chains], zero past d and past the launch's chains), for every
// shape: in registers it is G KF doubles beside 8 G JT of gacc and 8 G of eta, which at the envelope's corners
// (G JT = 16) is the whole register file; one placement also keeps the instantiations at one per (G, JT).
// The slot is released after the backward.
//
// A launch carries C <= 16 chains: the columns past C hold zero coefficients (eta = 0: finite work) and write no
// partials.  A column's sums depend on that column's coefficients alone, and the block reduction adds a chain's
// pieces in (lane group, wave) order, so a chain's lp and gradient are the same bits in whichever column and batch
// it runs, and however many shards share the launch.
//
// Envelope (stk_sweep_cat_supported): G <= 16, G ceil(d / 16) <= 16 -- K = 2 to d = 256, K = 3 to d = 128, K = 5 to
// d = 64, K = 9 to d = 32, K = 17 to d = 16.  Occupancy is two waves per SIMD where both the registers (cat_minb) and
// LDS (cat_waves) allow it, one otherwise; the comments there say which binds at which shape.
#include "sweep_common.h"
#include "launchers.h"
#include <math.h>
#include <algorithm>

namespace stk {

static_assert(CAT_MAX_CHAINS == SM_C, "a launch's chains are the MFMA's columns");
__host__ __device__ constexpr int cat_gb(int G) { return G > 14 ? 2 : G > 12 ? 4 : 8; }   // classes per forward pass over the sub-tile's columns
constexpr int CAT_RD_W = 16;                     // waves of the reduce: k_sweep_reduce's

// Two waves per SIMD (256 registers a lane) where the kernel was seen to fit them without scratch: gacc takes 8 G JT
// registers, eta / d eta 8 G, the d alpha sums 2 G, and the residual's temporaries and constants some 90 more.  Past
// that one wave per SIMD with the whole unified file (the MFMA's tuples in its accumulator half).
__host__ __device__ constexpr int cat_minb(int G, int KF) {
  const int lim = G == 1 ? 16 : G == 2 ? 8 : G == 3 ? 4 : G == 4 ? 3 : G == 5 ? 2 : G == 6 ? 1 : 0;   // the most 16-column tiles
  return KF / 4 <= lim ? 2 : 1;
}
__host__ __device__ constexpr size_t cat_lds_bytes_at(int G, int d, int NW) {
  const int JT = (d + 15) / 16;
  const size_t main = (size_t)NW * sweepm_slot_bytes(d) + sizeof(double) * (EX_TAB + (size_t)G * 16 * JT * 16 + (size_t)G * 16);
  const size_t red = sizeof(double) * ((size_t)G * 16 * JT * 16 + (size_t)(G + 1) * 16);
  return main > red ? main : red;
}
// Waves per block.  4, two blocks per CU, is k_sweep16's shape -- but LDS, not the registers, decides whether two
// blocks fit: the slots, the exp table and the beta image of a 4-wave block pass half the CU's 160 KB at G = 1 from
// d = 113 and at G = 2 from d = 81.  Where the registers allow two waves per SIMD and an 8-wave block (one beta image
// and one table for 8 slots) fits the CU at the tile count's largest d, the block is 8 waves: G = 1 at 112 < d <= 128,
// G = 2 at 80 < d <= 112.  Left at one wave per SIMD by LDS: G = 2 at 112 < d <= 128.  Past d = 128 (G = 1 alone) even
// 4 slots do not fit beside the beta image: 2 waves, two such blocks per CU up to d = 176 (one wave per SIMD), one past it.
__host__ __device__ constexpr int cat_waves(int G, int KF) {
  if (KF > 32) return 2;
  const int dmax = 4 * KF;
  if (cat_minb(G, KF) == 2 && 2 * cat_lds_bytes_at(G, dmax, 4) > BIG_LDS_BYTES && cat_lds_bytes_at(G, dmax, 8) <= BIG_LDS_BYTES) return 8;
  return 4;
}
__host__ __device__ constexpr size_t cat_lds_bytes(int G, int d) { return cat_lds_bytes_at(G, d, cat_waves(G, 4 * ((d + 15) / 16))); }
// Waves per SIMD the kernel is built for (__launch_bounds__' second argument): two where the registers allow them
// (cat_minb) AND the block shape cat_waves chose puts 8 waves on the CU at the tile count's largest d; else one, with
// the whole register file -- so the bound follows what LDS leaves (G = 2 at 112 < d <= 128 and G = 1 past d = 128 are
// one wave per SIMD whatever the registers would allow).
__host__ __device__ constexpr int cat_wpe(int G, int KF) {
  if (cat_minb(G, KF) == 1) return 1;
  const int NW = cat_waves(G, KF);
  const size_t blocks = BIG_LDS_BYTES / cat_lds_bytes_at(G, 4 * KF, NW);
  return blocks * NW >= 8 ? 2 : 1;
}

// exp(t) for t <= 0 (any t: it overflows to +inf past 709.78 on its own) by the table exp of gamma_resid: the same
// table, reduction and v_ldexp_f64 on clamp800(t), e^r = 1 + rr by the Taylor quartic (error r^5 / 120 < 4e-20, no
// mean over the interval, as gamma_resid's comment explains) and one fma.  t = 0 gives 1 exactly.  A NaN t gives a
// finite value (the clamp): the caller keeps the NaN by other means.
__device__ __forceinline__ double cat_exp(double t, const double* tab) {
  constexpr double MAGIC = 6755399441055744.0;            // 1.5 * 2^52
  constexpr double INV_L = 1477.3197218702985;            // 1024 / ln 2
  constexpr double L = 0.0006769015435155716;             // ln 2 / 1024
  const double c = clamp800(t);
  const double sn = fma(c, INV_L, MAGIC);
  const int ni = (int)(uint32_t)__builtin_bit_cast(uint64_t, sn);
  const double n = sn - MAGIC;
  const double r = fma(-n, L, c);
  const double rr = fma(r * r, fma(fma(1.0 / 24.0, r, 1.0 / 6.0), r, 0.5), r);
  const double T = __builtin_amdgcn_ldexp(tab[ni & (EX_TAB - 1)], ni >> 10);
  return fma(T, rr, T);
}

// The softmax residual of one (row, chain): eta[g] in, d eta_g out in its place; lm <- lm + eta_y - m, sp <- sp s.
// pz = sum_g 0 eta_g is 0 where every eta is finite, whatever its size, and NaN otherwise, and enters lp and every
// d eta_g, so a non-finite eta never leaves a finite number behind (the table exp alone would: its clamp turns a NaN
// into a finite argument).  Finite eta give t_g = eta_g - m <= 0, exactly 0 at the largest (e = 1), and e = 0 below
// -745 (t_g = -inf included, where two eta of about 1e308 and opposite signs meet: lp is then -inf, as its value is).
template <int G>
__device__ __forceinline__ void cat_resid(double (&eta)[G], int32_t y, bool valid, const double* tab, double& lm, double& sp) {
  double m = 0.0, pz = 0.0;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m = __builtin_fmax(m, eta[g]);
    pz = fma(eta[g], 0.0, pz);
  }
  double ey = 0.0;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    ey = y == g + 1 ? eta[g] : ey;
    eta[g] -= m;
  }
  double s = cat_exp(-m, tab);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    eta[g] = cat_exp(eta[g], tab);
    s += eta[g];
    if (G > 12 || (g & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // four exponentials in flight (one past G = 12): all G interleaved spill
  }
  const double ri = pd_rcp(s);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const double dv = fma(-eta[g], ri, y == g + 1 ? 1.0 : 0.0) + pz;
    eta[g] = valid ? dv : 0.0;
  }
  lm = valid ? lm + ((ey - m) + pz) : lm;
  sp = valid ? sp * s : sp;
}

template <int G, int KF>
__global__ __launch_bounds__(64 * cat_waves(G, KF), cat_wpe(G, KF)) void k_sweep_cat(SweepArgs A) {
  static_assert(G >= 1 && G <= 16 && KF % 4 == 0 && G * (KF / 4) <= 16, "k_sweep_cat: outside the envelope");
  constexpr int JT = KF / 4, KC = 16 * JT, NW = cat_waves(G, KF);
  const int shard = A.shard0 + blockIdx.x / A.G;
  const int chunk = blockIdx.x % A.G;
  if (A.req_step && A.req_step[shard] != A.step_id - 1) return;
  if (A.ran && chunk == 0 && threadIdx.x == 0) atomicAdd(&A.ran[A.step_id & 63], 1);
  const ShardDev sh = A.shards[shard];
  const int d = sh.d, C = A.C;
  const int tid = threadIdx.x, lane = tid & 63, w = uniform_int(tid >> 6);
  const int lr = lane & 15, lh = lane >> 4;
  const int64_t nt = (sh.n + 63) / 64;
  const int64_t t0 = nt * chunk / A.G, t1 = nt * (chunk + 1) / A.G;
  const int64_t r0 = t0 * 64, r1 = std::min<int64_t>(sh.n, t1 * 64);
  const int nrows = (int)(r1 - r0);
  const int nsub = (nrows + SM_R - 1) / SM_R;
  const int mine = nsub > w ? (nsub - w + NW - 1) / NW : 0;   // own sub-tiles u = w + NW k
  const int SBX = SM_R * d * 8;
  const int SS = sweepm_slot_bytes(d);

  extern __shared__ __attribute__((aligned(16))) double lds[];
  char* const slot = reinterpret_cast<char*>(lds) + (size_t)w * SS;
  double* const tab = reinterpret_cast<double*>(reinterpret_cast<char*>(lds) + (size_t)NW * SS);
  double* const Bs = tab + EX_TAB;                 // [G][KC columns][16 chains] beta, zero past d and past C
  double* const As = Bs + (size_t)G * KC * 16;     // [G][16 chains] alpha
  exp_table_init(tab);
  for (int i = tid; i < G * KC * 16; i += NW * 64) {
    const int c = i & 15, col = (i >> 4) % KC, g = (i >> 4) / KC;
    Bs[i] = (c < C && col < d) ? A.q[chain_row(A, shard, c) * A.Dp + G + g * d + col] : 0.0;
  }
  for (int i = tid; i < G * 16; i += NW * 64) {
    const int c = i & 15, g = i >> 4;
    As[i] = c < C ? A.q[chain_row(A, shard, c) * A.Dp + g] : 0.0;
  }
  __syncthreads();
  __builtin_amdgcn_s_waitcnt(0xF70);

  const __amdgpu_buffer_rsrc_t xr = uniform_rsrc(sh.x + r0 * d, (int64_t)nrows * d * 8);
  const __amdgpu_buffer_rsrc_t yr = uniform_rsrc(sh.yi + r0, (int64_t)nrows * 4);
  const int nx = (SBX + 1023) >> 10;
  const int last_lanes = (SBX - ((nx - 1) << 10)) >> 4;
  auto issue = [&](int k) {           // 1 KiB per DMA instruction, aux = 2 (nt), as k_sweep16
    const int u = w + NW * k;
    const int xoff = u * SBX;
    for (int j = 0; j < nx - 1; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_vptr)(slot + j * 1024), 16, lane * 16, xoff + j * 1024, 0, 2);
    if (lane < last_lanes)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_vptr)(slot + (nx - 1) * 1024), 16, lane * 16,
                                               xoff + (nx - 1) * 1024, 0, 2);
    if (lane < SM_R)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(yr, (lds_vptr)(slot + SBX), 4, lane * 4, u * SM_R * 4, 0, 2);
  };

  dbl4 gacc[G][JT];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int t = 0; t < JT; ++t) gacc[g][t] = dbl4{0.0, 0.0, 0.0, 0.0};
  double ga[G];                        // d lp / d alpha_g: the lane's sum of d eta_g
#pragma unroll
  for (int g = 0; g < G; ++g) ga[g] = 0.0;
  double lm = 0.0, sp = 1.0;
  int se = 0;                          // sum_i log s_i = log sp + se ln 2
  const double* xs = reinterpret_cast<const double*>(slot);
  const double* xrow = xs + lr * d;
  const double* bl = Bs + lh * 16 + lr;
  const double* al = As + lr;

  if (mine > 0) issue(0);
  for (int k = 0; k < mine; ++k) {
    __builtin_amdgcn_s_waitcnt(0xF70);                 // vmcnt(0): sub-tile k landed
    __builtin_amdgcn_sched_barrier(0);
    const int rv = std::min(SM_R, nrows - SM_R * (w + NW * k));
    // ---- forward: eta_g[row lh + 4i][chain lr] - alpha_g, cat_gb(G) classes at a time.  The accumulators start at the
    // MFMA's inline zero (the residual adds alpha_g: G splats of alpha would be 8 G registers beside the 8 G the first
    // k-step writes) and a group's tiles are copied out to plain registers before the next group runs: the MFMA's
    // tuples live in the accumulator half of the register file, which gacc fills on its own at G JT = 16.
    // One k-step's operands (a column of X, the group's betas) are read while the step before it runs on the MFMA,
    // and no further ahead: left to itself the scheduler hoists every LDS read of the sub-tile, G KF doubles of
    // registers.  16 (JT - 1) < d: only the last four k-steps can reach past column d - 1, where they meet a zero of
    // the beta image; those alone are clamped (a clamp with the runtime d costs an address register held across the loop).
    double de[G][4];
#pragma unroll
    for (int g0 = 0; g0 < G; g0 += cat_gb(G)) {
      constexpr int GBm = cat_gb(G) < G ? cat_gb(G) : G;
      const int gn = G - g0 < GBm ? G - g0 : GBm;      // a compile-time value once unrolled
      dbl4 ea[GBm];
      auto fwd_load = [&](int s, double& xa, double (&bv)[GBm]) {
        xa = xrow[s < KF - 4 ? 4 * s + lh : std::min(4 * s + lh, d - 1)];
#pragma unroll
        for (int g = 0; g < GBm; ++g)
          if (g < gn) bv[g] = bl[((g0 + g) * KC + 4 * s) * 16];
      };
      double xn, bn[GBm];
      fwd_load(0, xn, bn);
#pragma unroll
      for (int s = 0; s < KF; ++s) {
        const double xa = xn;
        double bc[GBm];
#pragma unroll
        for (int g = 0; g < GBm; ++g) bc[g] = bn[g];
        if (s + 1 < KF) fwd_load(s + 1, xn, bn);
#pragma unroll
        for (int g = 0; g < GBm; ++g)
          if (g < gn) ea[g] = mfma_f64(xa, bc[g], s == 0 ? dbl4{0.0, 0.0, 0.0, 0.0} : ea[g]);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int g = 0; g < GBm; ++g)
        if (g < gn) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            de[g0 + g][i] = ea[g][i];
            if constexpr (G > cat_gb(G)) asm volatile("" : "+v"(de[g0 + g][i]));
          }
        }
      __builtin_amdgcn_sched_barrier(0);
    }
    int32_t yv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) yv[i] = *reinterpret_cast<const int32_t*>(slot + SBX + (lh + 4 * i) * 4);
    // ---- residual: d eta takes eta's place
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double e[G];
#pragma unroll
      for (int g = 0; g < G; ++g) e[g] = de[g][i] + al[g * 16];
      cat_resid<G>(e, yv[i], lh + 4 * i < rv, tab, lm, sp);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        de[g][i] = e[g];
        ga[g] += e[g];
      }
      __builtin_amdgcn_sched_barrier(0);   // one row's temporaries at a time: interleaved, the four rows spill
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- backward: one A operand per (k-step, column tile) serves the G classes; read one step ahead, as the forward's
    auto bwd_load = [&](int u) {
      const int s = u / JT, t = u % JT;
      return xs[(lh + 4 * s) * d + (t < JT - 1 ? 16 * t + lr : std::min(16 * t + lr, d - 1))];
    };
    {
      double xn = bwd_load(0);
#pragma unroll
      for (int u = 0; u < 4 * JT; ++u) {
        const double xa = xn;
        if (u + 1 < 4 * JT) xn = bwd_load(u + 1);
#pragma unroll
        for (int g = 0; g < G; ++g) gacc[g][u % JT] = mfma_f64(xa, de[g][u / JT], gacc[g][u % JT]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);                // lgkmcnt(0): the slot is free
    __builtin_amdgcn_sched_barrier(0);
    if (k + 1 < mine) issue(k + 1);
    __builtin_amdgcn_sched_barrier(0);
    // renormalise the running product: its exponent moves to an integer, exactly (no log in the loop, no rounding)
    se += __builtin_amdgcn_frexp_exp(sp);
    sp = __builtin_amdgcn_frexp_mant(sp);
  }
  double lpa = lm - fma((double)se, 0.6931471805599453, log(sp));

  // ---- fixed-order block reduction -> one partial row per chain.  The scalar sums: the four lane groups of a
  // wave by two exchanges ((lh 0 + 1) + (lh 2 + 3), whichever lane), then the waves in wave order through LDS, as
  // the gradient tiles.
  lpa += __shfl_xor(lpa, 16);
  lpa += __shfl_xor(lpa, 32);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    ga[g] += __shfl_xor(ga[g], 16);
    ga[g] += __shfl_xor(ga[g], 32);
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __syncthreads();
  double* red = lds;                                   // [G][KC columns][16 chains]
  double* reds = red + (size_t)G * KC * 16;            // [G + 1][16 chains]: d alpha_g, lp
  for (int ww = 0; ww < NW; ++ww) {
    if (w == ww) {
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int t = 0; t < JT; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            double* p = red + ((size_t)(g * KC + 16 * t + lh + 4 * i)) * 16 + lr;
            *p = ww == 0 ? gacc[g][t][i] : *p + gacc[g][t][i];
          }
      if (lane < 16) {
#pragma unroll
        for (int g = 0; g < G; ++g) reds[g * 16 + lr] = ww == 0 ? ga[g] : reds[g * 16 + lr] + ga[g];
        reds[G * 16 + lr] = ww == 0 ? lpa : reds[G * 16 + lr] + lpa;
      }
    }
    __syncthreads();
  }
  double* out = A.partial + ((size_t)shard * A.Gs + chunk) * C * A.PW;
  const int gd = G * d;
  for (int i = tid; i < C * gd; i += NW * 64) {
    const int c = i / gd, o = i - c * gd, g = o / d, j = o - g * d;
    out[(size_t)c * A.PW + G + o] = red[((size_t)(g * KC + j)) * 16 + c];
  }
  for (int i = tid; i < C * (G + 1); i += NW * 64) {
    const int c = i / (G + 1), o = i - c * (G + 1);
    out[(size_t)c * A.PW + (o < G ? o : G + gd)] = reds[o * 16 + c];
  }
}

// The reduce: chunk partials summed in reduce_chunk_range's order (sweep.hip: CAT_RD_W waves each sum a contiguous
// range of the chunks in order, 8 loads in flight; then the waves in wave order), the normal(0, s) priors on every
// alpha_g (pa) and every beta entry (pb), lp and the gradient written straight into [chain][Dp] in the q layout.
// Flat priors change no bit.  grid (nshards * C, ceil(PW / 64)), PW = G (d + 1) + 1.
__global__ __launch_bounds__(64 * CAT_RD_W) void k_sweep_reduce_cat(SweepArgs A, double* lp_out, double* g_out, int C, int G) {
  const int gidl = blockIdx.x;
  const int shard = A.shard0 + gidl / C, c = gidl % C;
  if (A.req_step && A.req_step[shard] != A.step_id - 1) return;
  const ShardDev sh = A.shards[shard];
  const int D = A.PW - 1;
  const int o = blockIdx.y * 64 + (threadIdx.x & 63);
  const int w = threadIdx.x >> 6;
  __shared__ double part[CAT_RD_W][64];
  const double v = o < A.PW ? reduce_chunk_range<CAT_RD_W>(A, shard, c, C, o, w) : 0.0;
  part[w][threadIdx.x & 63] = v;
  __syncthreads();
  if (w != 0 || o >= A.PW) return;
  double t = part[0][threadIdx.x];
#pragma unroll
  for (int i = 1; i < CAT_RD_W; ++i) t += part[i][threadIdx.x];
  const size_t gid = chain_row(A, shard, c);
  const double* qc = A.q + gid * A.Dp;
  const bool flat = sh.pa == 0.0 && sh.pb == 0.0;
  if (o < D) {
    g_out[gid * A.Dp + o] = flat ? t : t - (o < G ? sh.pa : sh.pb) * qc[o];
  } else {
    double prior_lp = 0.0;
    if (!flat) {
      double sa = 0.0, sb = 0.0;
      for (int j = 0; j < G; ++j) sa = fma(qc[j], qc[j], sa);
      for (int j = G; j < D; ++j) sb = fma(qc[j], qc[j], sb);
      prior_lp = -0.5 * (sh.pa * sa + sh.pb * sb);
    }
    lp_out[gid] = t + prior_lp;
  }
}

// y in [1, K] of a categorical shard (stk_model_set_categories), the sibling of datagen.hip's k_check_y01: *first =
// the first row whose class is outside, or the value it was set to.
__global__ __launch_bounds__(256) void k_check_ycat(const int32_t* y, int64_t n, int K, unsigned long long* first) {
  __shared__ unsigned long long m[4];
  const unsigned long long none = ~0ull >> 1;
  unsigned long long b = none;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int32_t v = y[i];
    if ((v < 1 || v > K) && (unsigned long long)i < b) b = (unsigned long long)i;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(b, o);
    b = t < b ? t : b;
  }
  if ((threadIdx.x & 63) == 0) m[threadIdx.x >> 6] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) b = m[w] < b ? m[w] : b;
    if (b != none) atomicMin(first, b);
  }
}

}  // namespace stk

using namespace stk;

// The envelope: G = K - 1 classes' tiles times the 16-column tiles of d fit 16 accumulator tiles.
bool stk_sweep_cat_supported(int G, int d) { return G >= 1 && G <= 16 && d >= 1 && G * ((d + 15) / 16) <= 16; }

// Kind 8's shape over n rows of d covariates for C <= 16 chains at K classes: k_sweep16's chunks (of (n, d) alone).
SweepLaunch stk_sweep_plan_cat(int64_t n, int d, int C, int ncat) {
  SweepLaunch p{};
  p.C = C;
  p.d = d;
  if (n < 1 || C < 1 || C > CAT_MAX_CHAINS || !stk_sweep_cat_supported(ncat - 1, d)) return p;
  if ((n * d * 8) / 512 >= ((int64_t)1 << 30)) return p;   // chunk bytes fit a buffer descriptor
  const int64_t nt = (n + 63) / 64;
  p.kind = SWEEP_CAT;
  p.T = 64;
  p.G = (int)std::max<int64_t>(1, std::min<int64_t>(512, (nt + 7) / 8));
  p.ld = ncat;
  p.waves = cat_waves(ncat - 1, 4 * ((d + 15) / 16));
  p.lds = cat_lds_bytes(ncat - 1, d);
  return p;
}

int stk_sweep_cat_pw(int ncat, int d) { return (ncat - 1) * (d + 1) + 1; }

// The one carrier of the class count through a launch: SweepLaunch::ld (launchers.h), handed on as SweepArgs.LD.
static int cat_ncat(const SweepLaunch& p) { return p.ld; }
static int cat_classes(const SweepLaunch& p) { return p.ld - 1; }   // G, the free classes

template <int G, int KF>
static hipError_t go_cat(const SweepArgs& A, int nblocks, size_t lds, hipStream_t st) {
  auto kern = k_sweep_cat<G, KF>;
  if (const hipError_t e = allow_big_lds((const void*)kern)) return e;
  hipLaunchKernelGGL(kern, dim3(nblocks), dim3(64 * cat_waves(G, KF)), lds, st, A);
  return hipGetLastError();
}

static SweepArgs cat_args(const SweepLaunch& p, int shard0, const SweepCall& c) {
  SweepArgs A{c.shards, c.q, c.partial, c.req_step, c.step_id, p.C, c.Dp, p.G, cat_ncat(p), stk_sweep_cat_pw(cat_ncat(p), p.d), shard0, c.Gs, c.ran};
  A.Ct = c.Ct;
  A.c0 = c.c0;
  return A;
}

hipError_t stk_launch_sweep_cat(const SweepLaunch& p, int shard0, int nsh, const SweepCall& c, hipStream_t st) {
  const int G = cat_classes(p), JT = (p.d + 15) / 16;
  if (p.kind != SWEEP_CAT || !stk_sweep_cat_supported(G, p.d) || p.C < 1 || p.C > CAT_MAX_CHAINS || p.lds != cat_lds_bytes(G, p.d) ||
      p.lds > BIG_LDS_BYTES)
    return hipErrorInvalidValue;
  const SweepArgs A = cat_args(p, shard0, c);
  const int nblocks = nsh * p.G;
  switch (G * 32 + JT) {
#define CAT_CASE(GG, JJ) case GG * 32 + JJ: return go_cat<GG, 4 * JJ>(A, nblocks, p.lds, st);
    CAT_CASE(1, 1) CAT_CASE(1, 2) CAT_CASE(1, 3) CAT_CASE(1, 4) CAT_CASE(1, 5) CAT_CASE(1, 6) CAT_CASE(1, 7) CAT_CASE(1, 8)
    CAT_CASE(1, 9) CAT_CASE(1, 10) CAT_CASE(1, 11) CAT_CASE(1, 12) CAT_CASE(1, 13) CAT_CASE(1, 14) CAT_CASE(1, 15) CAT_CASE(1, 16)
    CAT_CASE(2, 1) CAT_CASE(2, 2) CAT_CASE(2, 3) CAT_CASE(2, 4) CAT_CASE(2, 5) CAT_CASE(2, 6) CAT_CASE(2, 7) CAT_CASE(2, 8)
    CAT_CASE(3, 1) CAT_CASE(3, 2) CAT_CASE(3, 3) CAT_CASE(3, 4) CAT_CASE(3, 5)
    CAT_CASE(4, 1) CAT_CASE(4, 2) CAT_CASE(4, 3) CAT_CASE(4, 4)
    CAT_CASE(5, 1) CAT_CASE(5, 2) CAT_CASE(5, 3)
    CAT_CASE(6, 1) CAT_CASE(6, 2) CAT_CASE(7, 1) CAT_CASE(7, 2) CAT_CASE(8, 1) CAT_CASE(8, 2)
    CAT_CASE(9, 1) CAT_CASE(10, 1) CAT_CASE(11, 1) CAT_CASE(12, 1) CAT_CASE(13, 1) CAT_CASE(14, 1) CAT_CASE(15, 1) CAT_CASE(16, 1)
#undef CAT_CASE
  }
  return hipErrorInvalidValue;
}

hipError_t stk_launch_sweep_reduce_cat(const SweepLaunch& p, int shard0, int nsh, const SweepCall& c, double* lp_out,
                                       double* g_out, hipStream_t st) {
  if (p.kind != SWEEP_CAT) return hipErrorInvalidValue;
  SweepArgs A = cat_args(p, shard0, c);
  A.ran = nullptr;
  hipLaunchKernelGGL(k_sweep_reduce_cat, dim3(nsh * p.C, (A.PW + 63) / 64), dim3(64 * CAT_RD_W), 0, st, A, lp_out, g_out,
                     p.C, cat_classes(p));
  return hipGetLastError();
}

hipError_t stk_launch_check_ycat(const int32_t* y, int64_t n, int K, int64_t* first, hipStream_t st) {
  if (const hipError_t e = hipMemsetAsync(first, 0x7f, sizeof(int64_t), st)) return e;   // past any row count
  int64_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_check_ycat, dim3((unsigned)blocks), dim3(256), 0, st, y, n, K, reinterpret_cast<unsigned long long*>(first));
  return hipGetLastError();
}
