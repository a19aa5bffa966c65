// Types and helpers shared by the regression sweeps (sweep.hip: C != 16 and the 64-chain GEMM
// passes; sweep16.hip: the 16-chain fp64-MFMA sweep; sweep16w.hip: its K-split for d > 128) and by
// the measurement tools in tools/.
#pragma once
#include "common.h"
#include "predictive_math.h"
#include "negbin_math.h"
#include "student_math.h"
#include "gamma_math.h"

// Which families' instantiations of the sweep kernels a translation unit of sweep.hip, sweep16.hip or
// sweep16w.hip holds.  Undefined: every family, instantiated implicitly where it is
// used -- a stand-alone tool that includes the kernel files as one translation unit.  The library's
// Makefile compiles each kernel file five times: -DSTK_SWEEP_TU=0 is the base object (what is not a
// template, and the logistic and linear families), 4, 5, 6 and 7 hold the Poisson, negative-binomial,
// Student-t and gamma families alone, so that a new family leaves the others' code objects as they were.  The
// preprocessor cannot read the STK_* enumerators, hence the numbers.
#ifdef STK_SWEEP_TU
static_assert(STK_POISSON == 4 && STK_NEGBIN == 5 && STK_STUDENT == 6 && STK_GAMMA == 7, "the Makefile's -DSTK_SWEEP_TU ids are the family ids");
static_assert(STK_SWEEP_TU == 0 || STK_SWEEP_TU == STK_POISSON || STK_SWEEP_TU == STK_NEGBIN || STK_SWEEP_TU == STK_STUDENT ||
                  STK_SWEEP_TU == STK_GAMMA,
              "STK_SWEEP_TU: 0 or a family with an object of its own");
#endif
#if !defined(STK_SWEEP_TU) || STK_SWEEP_TU == 0
#define STK_SWEEP_BASE 1   // this translation unit defines what is not a template
#endif
// After the definition of a launcher template `template <int FAM> hipError_t F(...)` (declared in
// launchers.h): F's instantiations in this translation unit, its parameter types as the arguments.  The
// base object declares the other families' `extern`, so that its dispatch finds them at link time and
// instantiates none of their kernels.
#if !defined(STK_SWEEP_TU)
#define STK_SWEEP_INSTANTIATE(F, ...)
#elif STK_SWEEP_TU == 0
#define STK_SWEEP_INSTANTIATE(F, ...)                          \
  template hipError_t F<STK_LOGREG>(__VA_ARGS__);              \
  template hipError_t F<STK_LINREG>(__VA_ARGS__);              \
  extern template hipError_t F<STK_POISSON>(__VA_ARGS__);      \
  extern template hipError_t F<STK_NEGBIN>(__VA_ARGS__);       \
  extern template hipError_t F<STK_STUDENT>(__VA_ARGS__);     \
  extern template hipError_t F<STK_GAMMA>(__VA_ARGS__);
#else
#define STK_SWEEP_INSTANTIATE(F, ...) template hipError_t F<STK_SWEEP_TU>(__VA_ARGS__);
#endif

namespace stk {

// A family is a residual, not a kernel: every sweep takes FAM and must know it.  What the kernels and
// their launchers ask about a family, in one place:
__host__ __device__ constexpr bool fam_known(int f) {
  return f == STK_LINREG || f == STK_LOGREG || f == STK_POISSON || f == STK_NEGBIN || f == STK_STUDENT || f == STK_GAMMA;
}
__host__ __device__ constexpr bool fam_yint(int f) { return f == STK_LOGREG || f == STK_POISSON || f == STK_NEGBIN; }   // y is the shard's int32 y_int
// The scalar next to beta, q[d + 1], as the kernels carry it per chain in their inv_s slot: linear
// 1 / sigma = exp(-u); negative binomial v = log phi itself, with phi = exp(v) kept beside it (once per
// chain, not per element); student_t 1 / sigma as linear (its y is the shard's double y too; nu, nu + 1 and
// 1 / nu are wave-uniform, read once from the shard's entry); gamma the shape a = exp(u) (fam_chain_scalar below);
// the others have none.
__host__ __device__ constexpr bool fam_inv_sigma(int f) { return f == STK_LINREG || f == STK_STUDENT; }
// A third partial sum per chain, column d + 2: the negative binomial's unweighted sum of sp(t), student_t's
// sum of z^2 / (nu + z^2).  Their residuals are also the heavy ones (a log1p and a reciprocal per element).
// The gamma family has none: its reduce finishes lp and d lp / d u from H = sum h(t) alone, the lp column.
__host__ __device__ constexpr bool fam_sum3(int f) { return f == STK_NEGBIN || f == STK_STUDENT; }
// The MFMA sweeps keep the exp table in LDS for the families whose residual takes an exp: those with an int32 y,
// and the gamma family, the one family with the table and a double y.
__host__ __device__ constexpr bool fam_exp_table(int f) { return fam_yint(f) || f == STK_GAMMA; }
// The gamma family's per-row stream is not the shard's y but ly = log y, computed once at model creation
// (capi_model.hip): ShardDev::sigma, which no other regression reads as an array, points at it.  Its per-chain
// scalar is the shape a = exp(u) itself, in the inv_s slot.
template <int FAM>
__device__ __forceinline__ const double* fam_ydouble(const ShardDev& sh) { return FAM == STK_GAMMA ? sh.sigma : sh.y; }
// The per-chain scalar of the inv_s slot from the chain's q[d + 1].
template <int FAM>
__device__ __forceinline__ double fam_chain_scalar(double q) {
  return fam_inv_sigma(FAM) ? exp(-q) : FAM == STK_GAMMA ? exp(q) : FAM == STK_NEGBIN ? q : 0.0;
}

typedef double dbl2 __attribute__((ext_vector_type(2)));   // loads from any address space

struct SweepArgs {
  const ShardDev* shards;
  const double* q;        // [nshards*Ct][Dp] evaluation points; this launch: rows shard*Ct + c0 + c, c < C
  double* partial;        // [nshards][G][C][PW]
  const int* req_step;    // nullptr: always run
  int step_id;
  int C, Dp, G, LD, PW;
  int shard0;             // first shard of this launch
  int Gs;                 // partial-buffer stride in chunks per shard (>= G)
  int* ran;               // optional: ran[step_id & 63] = 1 when any shard swept
  double* qT;             // v5 workspace: [nshards][KP][64] swizzled beta^T images (KP = d rounded to 32)
  double* R;              // v5 workspace: [nshards][Rrows][64] residuals d eta, swizzled rows
  int64_t Rrows;          // v5: rows of R per shard (n rounded up to 64)
  int Ct;                 // chains per shard in q / lp / grad (C when the launch is the shard's only batch)
  int c0;                 // first chain of this launch's batch within its shard
};

// Row of chain c of the launch's batch in q, lp_out and g_out.
__device__ __forceinline__ size_t chain_row(const SweepArgs& A, int shard, int c = 0) {
  return (size_t)shard * A.Ct + A.c0 + c;
}

__device__ __forceinline__ void wait_vmcnt(int n) {
  // s_waitcnt encoding (gfx9): vmcnt [3:0] + [15:14], expcnt [6:4] = 7, lgkmcnt [11:8] = 15
#define STK_VMCNT(N) case N: __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | 0xF70); break;
  switch (n) {   // vmcnt is 6 bits on gfx950: 0..63
    STK_VMCNT(0) STK_VMCNT(1) STK_VMCNT(2) STK_VMCNT(3) STK_VMCNT(4) STK_VMCNT(5) STK_VMCNT(6)
    STK_VMCNT(7) STK_VMCNT(8) STK_VMCNT(9) STK_VMCNT(10) STK_VMCNT(11) STK_VMCNT(12) STK_VMCNT(13)
    STK_VMCNT(14) STK_VMCNT(15) STK_VMCNT(16) STK_VMCNT(17) STK_VMCNT(18) STK_VMCNT(19) STK_VMCNT(20)
    STK_VMCNT(21) STK_VMCNT(22) STK_VMCNT(23) STK_VMCNT(24) STK_VMCNT(25) STK_VMCNT(26) STK_VMCNT(27)
    STK_VMCNT(28) STK_VMCNT(29) STK_VMCNT(30) STK_VMCNT(31) STK_VMCNT(32) STK_VMCNT(33) STK_VMCNT(34)
    STK_VMCNT(35) STK_VMCNT(36) STK_VMCNT(37) STK_VMCNT(38) STK_VMCNT(39) STK_VMCNT(40) STK_VMCNT(41)
    STK_VMCNT(42) STK_VMCNT(43) STK_VMCNT(44) STK_VMCNT(45) STK_VMCNT(46) STK_VMCNT(47) STK_VMCNT(48)
    STK_VMCNT(49) STK_VMCNT(50) STK_VMCNT(51) STK_VMCNT(52) STK_VMCNT(53) STK_VMCNT(54) STK_VMCNT(55)
    STK_VMCNT(56) STK_VMCNT(57) STK_VMCNT(58) STK_VMCNT(59) STK_VMCNT(60) STK_VMCNT(61) STK_VMCNT(62)
    STK_VMCNT(63)
    default: __builtin_amdgcn_s_waitcnt(0xF70); break;   // vmcnt(0)
  }
#undef STK_VMCNT
}

template <int N>
__device__ __forceinline__ void wait_vm() { __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | 0xF70); }

typedef double dbl4 __attribute__((ext_vector_type(4)));
constexpr int SM_W = 4;                 // waves per block (one per SIMD)
constexpr int SM_R = 16;                // rows per wave sub-tile = MFMA M (forward) and K (backward)
constexpr int SM_C = 16;                // chains per launch row = MFMA N
constexpr int SM_MINB = 2;              // blocks per CU: two waves per SIMD (one wave cannot cover the slot's DMA latency)
__host__ __device__ constexpr int sweepm_slot_bytes(int d) { return SM_R * d * 8 + 128; }

__device__ __forceinline__ dbl4 mfma_f64(double a, double b, dbl4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// 64-bit select as an integer bit blend (v_bfi_b32 x 2): a C++ conditional here lets the
// compiler sink a whole arm's arithmetic into an exec-masked branch, which serialises the
// four (row, chain) pairs of a lane instead of interleaving them
__device__ __forceinline__ double blend(uint32_t m, double a, double b) {   // m = ~0u: a, 0: b
  const uint64_t ua = __builtin_bit_cast(uint64_t, a), ub = __builtin_bit_cast(uint64_t, b);
  const uint64_t mm = ((uint64_t)m << 32) | m;
  return __builtin_bit_cast(double, (ua & mm) | (ub & ~mm));
}

// exp table: T_j = 2^(j/1024), j < 1024 (8 KB of LDS per workgroup)
constexpr int EX_TAB = 1024;
__device__ void exp_table_init(double* tab) {
  for (int i = threadIdx.x; i < EX_TAB; i += blockDim.x) tab[i] = exp2((double)i / (double)EX_TAB);
}

// Logistic residual v4: Stan 2.19's bernoulli_logit term and its derivative for one (row,
// chain), t = (2y - 1) eta:
//   t > 20:   lt = -exp(-t),             dv/sgn = exp(-t)
//   t < -20:  lt = t,                    dv/sgn = 1
//   else:     lt = -log1p(exp(-t)),      dv/sgn = exp(-t) / (exp(-t) + 1)
// computed branch-free from e = exp(-|t|) as lt = min(t, 0) - log1p(e), dv/sgn = (t < 0 ?
// 1/(1+e) : e/(1+e)); above 20 the smooth form differs from Stan's by <= e^2/2 < 2.2e-18.
// The kernel works with s = -t = (1 - 2y) eta, whose sign bit is eta's plus y << 31 (one
// v_lshl_add_u32: adding 2^31 to the high word flips the sign), and returns -dv the same way;
// the kernel negates the gradient sums once at the end.
//
// The log is not taken per element.  Per lane (one chain) the kernel keeps
//   lm = sum (t - |t|)              = 2 sum min(t, 0), exact per term, a NaN eta stays NaN
//   sp = prod (1 + e) - 1           one fma per element: sp <- sp (1 + e) + e
// and adds log1p(sp) to the lane's lp every 64 sub-tiles (256 elements: 1 + sp < 2^256, and
// every step adds at most eps of relative error to 1 + sp, so log1p(sp) is off by <= 256 eps
// absolute); lp = lm/2 - sum log1p(sp).  Rows with e below eps are summed exactly (1 + e = 1,
// sp += e).  Against residual v3 this drops the table log1p (its index, two LDS reads, a degree-4
// polynomial) and the per-element lp terms: ~27 instead of ~43 vector instructions per element.
//   exp(-a), a = min(|t|, 700): n = rint(-a 1024/ln2) by the 1.5 2^52 trick, r = -a - n ln2/1024
//   (|r| <= ln2/2048; ln2/1024 rounded once: |error of r| <= n ulp(ln2/1024)/2, 1.6e-15 relative at
//   a = 20), e^r by a fitted degree-3 polynomial (relative error 9.4e-17), times T_{n mod 1024}, times
//   2^{n div 1024} by v_ldexp_f64 -- whose exponent is -1100 for t < -20, making e = 0: then
//   lt = min(t, 0) = t and dv/sgn = 1/(1 + 0) = 1 exactly, Stan's lower branch;
//   1/(1 + e): v_rcp_f64 + one Newton step (11 ulp, tools/rcp_acc.hip).
__device__ __forceinline__ double fmin_abs(double x, double c) {   // min(|x|, c), NaN x -> c
  // one v_min_f64 with the abs modifier (fmin() adds a canonicalising v_max_f64 in IEEE mode)
  double r;
  asm("v_min_f64 %0, |%1|, %2" : "=v"(r) : "v"(x), "s"(c));
  return r;
}
__device__ __forceinline__ double logit_resid4(double eta, uint32_t y, const double* tab, double& lm, double& sp) {
  constexpr double MAGIC = 6755399441055744.0;            // 1.5 * 2^52
  constexpr double INV_L = 1477.3197218702985;            // 1024 / ln 2
  constexpr double L = 0.0006769015435155716;             // ln 2 / 1024
  constexpr double C2 = 0.5000000039583942, C3 = 0.16666666713444417;   // e^r on |r| <= ln2/2048 (fit)
  const uint64_t eb = __builtin_bit_cast(uint64_t, eta);
  const double s = __builtin_bit_cast(double, (eb & 0xFFFFFFFFull) | ((uint64_t)((y << 31) + (uint32_t)(eb >> 32)) << 32));
  const double a = fmin_abs(s, 700.0);                    // |s| = |eta|; NaN -> 700 (the NaN stays in lm)
  const double sn = fma(-a, INV_L, MAGIC);
  const int ni = (int)(uint32_t)__builtin_bit_cast(uint64_t, sn);
  const double n = sn - MAGIC;
  const double r = fma(-n, L, -a);
  const double p = fma(fma(fma(C3, r, C2), r, 1.0), r, 1.0);
  const int ke = (s > 20.0) ? -1100 : (ni >> 10);         // Stan's lower cutoff (t < -20): e = 0
  const double e = __builtin_amdgcn_ldexp(tab[ni & (EX_TAB - 1)] * p, ke);
  const double u = 1.0 + e;
  double ri = __builtin_amdgcn_rcp(u);
  ri = fma(ri, fma(-u, ri, 1.0), ri);
  const double w = e * ri;
  const uint64_t sb = __builtin_bit_cast(uint64_t, s);
  const uint32_t spos = (uint32_t)((int32_t)(sb >> 32) >> 31);   // ~0u when s < 0, i.e. t > 0
  const uint64_t dvp = __builtin_bit_cast(uint64_t, blend(spos, w, ri));   // dv/sgn
  lm += -s - fabs(s);                                     // t - |t|
  sp = fma(sp, u, e);
  return __builtin_bit_cast(double, (dvp & 0xFFFFFFFFull) | ((uint64_t)((y << 31) + (uint32_t)(dvp >> 32)) << 32));   // -dv
}

// Poisson residual: Stan 2.19's poisson_log term (propto: no lgamma(y + 1)) and its derivative for
// one (row, chain), mu = exp(eta):
//   lt = y eta - mu,   dv = y - mu        (returned; lm <- fma(y, eta, lm - mu))
// mu by the table exp of logit_resid4 (same table, same degree-3 polynomial, v_ldexp_f64) on
// a = min(max(eta, -800), 800): n = rint(a 1024/ln2) by the 1.5 2^52 trick (valid for moderate
// arguments only, hence the clamp; |n| < 2^21), r = a - n ln2/1024, mu = T_{n mod 1024} e^r
// 2^{n div 1024}, which overflows to +inf past eta = 709.78 and underflows to 0 on its own.  eta
// itself enters y eta unclamped and a NaN eta (the clamp turns it into a finite a) stays NaN in lm
// through the fma, so where a row's exp overflows the lane's lp is -inf, or NaN when y eta
// overflowed too, never a finite number.  No reciprocal, no running product, no flush: 18 vector
// instructions per element (the sum of dv included) against v4's ~27.
__device__ __forceinline__ double clamp800(double x) {   // NaN x -> -800
  // v_max_f64 + v_min_f64 (fmax() / fmin() add a canonicalising v_max_f64 each in IEEE mode)
  double r;
  asm("v_max_f64 %0, %1, %2\n\tv_min_f64 %0, %0, %3" : "=&v"(r) : "v"(x), "s"(-800.0), "s"(800.0));
  return r;
}
__device__ __forceinline__ double pois_resid(double eta, int32_t y, const double* tab, double& lm) {
  constexpr double MAGIC = 6755399441055744.0;            // 1.5 * 2^52
  constexpr double INV_L = 1477.3197218702985;            // 1024 / ln 2
  constexpr double L = 0.0006769015435155716;             // ln 2 / 1024
  constexpr double C2 = 0.5000000039583942, C3 = 0.16666666713444417;   // e^r on |r| <= ln2/2048 (fit)
  const double yd = (double)y;                            // v_cvt_f64_i32: exact for every int32
  const double a = clamp800(eta);
  const double sn = fma(a, INV_L, MAGIC);
  const int ni = (int)(uint32_t)__builtin_bit_cast(uint64_t, sn);
  const double n = sn - MAGIC;
  const double r = fma(-n, L, a);
  const double p = fma(fma(fma(C3, r, C2), r, 1.0), r, 1.0);
  const double mu = __builtin_amdgcn_ldexp(tab[ni & (EX_TAB - 1)] * p, ni >> 10);
  lm = fma(yd, eta, lm - mu);
  return yd - mu;
}

// Negative-binomial residual: Stan's neg_binomial_2_log term in the form of include/stark_hip.h
// (STK_NEGBIN) and its derivative for one (row, chain), t = eta - v, v = log phi:
//   lt = y eta - (y + phi) sp(t),   dv = y - (y + phi) sigma(t)     (returned)
//   lm <- lm + lt,  ss <- ss + sp(t)     (ss: the unweighted sum the v gradient needs)
// The phi-only terms (sum_j log1p(j / phi), the digamma difference) are not here: k_sweep_reduce adds
// them once per (shard, chain) from the shard's count table (negbin_math.h).
// From e = exp(-|t|) by the table exp of logit_resid4 (|t| clamped to 800, where e is 0):
//   sp(t) = max(t, 0) + log1p(e)     max(t, 0) as (t + |t|) / 2: a NaN t stays NaN, t = +inf gives +inf
//   lt = y eta - (y + phi) log1p(e) (t < 0),  y v - phi t - (y + phi) log1p(e) (t >= 0)
// -- for t >= 0 the product (y + phi) t is multiplied out and y eta - y t = y v taken exactly: at |eta| ~ 1e150 and a
// count of 2^31 the two products would cancel seven digits of lp.  The y v this leaves cancels against the table's
// sum_j T_j log1p(j / phi) only where |v| is large, and then to within eps |v| of lp.
//   dv = (y e - phi) / (1 + e) (t >= 0), (y - phi e) / (1 + e) (t < 0)     v_rcp_f64 + two Newton steps
// -- y - (y + phi) sigma(t) with sigma(t) = 1 / (1 + e) or e / (1 + e) multiplied out, so that a count of 2^31
// does not turn the last ulp of sigma into 2e-7 of d eta: what cancels is y e against phi, both to an ulp.
// log1p(e) by pd_log1p01 (predictive_math.h: e in [0, 1], relative accuracy kept as e -> 0, so
// (y + phi) sp(t) -> mu (1 + y / phi) at large phi without a switch to Poisson).  The weight y + phi
// differs per row, so logit_resid4's running product cannot carry the weighted sum; with log1p(e)
// at hand the unweighted sum costs one add.  phi = inf (t = -inf) gives sp = NaN; phi = 0 leaves the
// sums finite and the reduce makes lp NaN.  About 74 vector instructions per element over the linear kernel's
// by the ISA count of k_sweep16<FAM, 25>, against 64 for logistic counted the same way.
__device__ __forceinline__ double negbin_resid(double eta, int32_t y, double v, double phi, const double* tab, double& lm,
                                               double& ss) {
  constexpr double MAGIC = 6755399441055744.0;            // 1.5 * 2^52
  constexpr double INV_L = 1477.3197218702985;            // 1024 / ln 2
  constexpr double L = 0.0006769015435155716;             // ln 2 / 1024
  constexpr double C2 = 0.5000000039583942, C3 = 0.16666666713444417;   // e^r on |r| <= ln2/2048 (fit)
  const double yd = (double)y;                            // v_cvt_f64_i32: exact for every int32
  const double t = eta - v;
  const double a = fmin_abs(t, 800.0);                    // NaN -> 800 (the NaN stays in sp through t)
  const double sn = fma(-a, INV_L, MAGIC);
  const int ni = (int)(uint32_t)__builtin_bit_cast(uint64_t, sn);
  const double n = sn - MAGIC;
  const double r = fma(-n, L, -a);
  const double p = fma(fma(fma(C3, r, C2), r, 1.0), r, 1.0);
  const double e = __builtin_amdgcn_ldexp(tab[ni & (EX_TAB - 1)] * p, ni >> 10);
  const uint32_t tneg = (uint32_t)((int32_t)(__builtin_bit_cast(uint64_t, t) >> 32) >> 31);   // ~0u when t < 0
  const double l1 = pd_log1p01(e);
  lm = fma(-(yd + phi), l1, lm) + blend(tneg, yd * eta, fma(yd, v, -phi * t));
  ss += fma(0.5, t, 0.5 * fabs(t)) + l1;
  const double num = blend(tneg, fma(-phi, e, yd), fma(yd, e, -phi));
  return num * pd_rcp(1.0 + e);
}

// The same terms with libm's exp and log1p, for the VALU sweeps (k_sweep, k_sweep2, k_sweep3: C <= 8),
// which keep no exp table.
__device__ __forceinline__ double negbin_resid_libm(double eta, double yd, double v, double phi, double& lm, double& ss) {
  const double t = eta - v;
  const double e = exp(-fabs(t));
  const double l1 = log1p(e);
  lm = fma(-(yd + phi), l1, lm) + (t < 0.0 ? yd * eta : fma(yd, v, -phi * t));
  ss += fma(0.5, t, 0.5 * fabs(t)) + l1;
  return (t < 0.0 ? fma(-phi, e, yd) : fma(yd, e, -phi)) / (1.0 + e);
}

// Student-t residual: Stan's student_t term under `~` with nu as data (include/stark_hip.h, STK_STUDENT) and
// its derivative for one (row, chain), z = (y - eta) / sigma, w = z^2 / nu:
//   lm <- lm + log1p(w)                 lp = -(nu + 1)/2 lm - n s + s, finished in the reduce
//   ss <- ss + z^2 / (nu + z^2)         d lp / d s = (nu + 1) ss - n + 1, finished in the reduce
//   dv = (nu + 1) z / (sigma (nu + z^2))        (returned)
// The constants lgamma((nu + 1)/2) - lgamma(nu/2) - log(nu pi)/2 are dropped, as Stan drops them; -log sigma per
// row is the reduce's -n s.  Nothing cancels: every term is a product or a quotient of non-negative numbers and
// z itself, so the relative error of each is a few ulp whatever the outlier (z = 1e3 at nu = 1) and whatever nu
// (nu = 1e6: w is tiny, st_log1p keeps its relative accuracy and (nu + 1)/2 log1p(z^2 / nu) -> z^2 / 2, the
// linear family's term).  nu, nu + 1 and 1 / nu are wave-uniform and come from the caller, read once per kernel.
// One reciprocal r = 1 / (nu + z^2) by pd_rcp (v_rcp_f64 + two Newton steps) serves ss = z^2 r and dv; the log1p
// is st_log1p (student_math.h: full range, one more reciprocal).  No exp, no table.
// Where z^2 overflows (|z| > 1.3e154) w = +inf: lm = +inf, so lp = -inf; r is NaN (pd_rcp's Newton step at 1/inf),
// so ss and dv are NaN: never a finite wrong number, and lp never +inf.  A NaN eta or sigma stays NaN throughout.
// 67 vector instructions per element over the linear kernel's by the ISA count of k_sweep16<FAM, 25>, against 74
// for the negative binomial counted the same way.
__device__ __forceinline__ double student_resid(double eta, double y, double inv_sigma, double nu, double nu1,
                                                double inv_nu, double& lm, double& ss) {
  const double z = (y - eta) * inv_sigma;
  const double z2 = z * z;
  lm += st_log1p(z2 * inv_nu);
  const double r = pd_rcp(nu + z2);
  ss = fma(z2, r, ss);
  return (z * r) * (nu1 * inv_sigma);
}

// The same terms with libm's log1p and a division, for the VALU sweeps (k_sweep, k_sweep2, k_sweep3: C <= 8).
__device__ __forceinline__ double student_resid_libm(double eta, double y, double inv_sigma, double nu, double nu1,
                                                     double inv_nu, double& lm, double& ss) {
  const double z = (y - eta) * inv_sigma;
  const double z2 = z * z;
  lm += log1p(z2 * inv_nu);
  const double r = 1.0 / (nu + z2);
  ss = fma(z2, r, ss);
  return (z * r) * (nu1 * inv_sigma);
}

// Gamma residual: Stan's gamma_lpdf(y | a, a exp(-eta)) in the deviance form of include/stark_hip.h (STK_GAMMA)
// and its derivative for one (row, chain), t = ly - eta with ly = log y the row's stream, a the chain's shape:
//   lm <- lm + h(t),  h(t) = e^t - 1 - t >= 0       lp = n kappa(a) - L - a H + u, finished in the reduce
//   dv = a (e^t - 1)                                 (returned)
// The textbook form n (a log a - lgamma a) + (a - 1) L - a sum (eta + y e^-eta) is not used: on precise data
// (shape 1e4 and up) a n and a L cancel and lp misses 1e-10 in fp64 whatever the kernel does.  Here nothing of
// the shape's size is subtracted: h >= 0 is summed as it is, and the reduce multiplies H by a once.
// e^t - 1 by the table exp of pois_resid (same table, same reduction, v_ldexp_f64) on clamp800(t), with two changes
// that the sum over the rows needs.  With T = T_{n mod 1024} 2^{n div 1024} and e^r = 1 + rr,
//   e^t - 1 = (T - 1) + T rr      one fma; T - 1 is exact for t in [-0.69, 0.69], where the difference cancels
//   rr = r + r^2 (1/2 + r (1/6 + r / 24))      Taylor to r^4: error r^5 / 120 < 4e-20
// pois_resid's fitted cubic is within 9.4e-17 of e^r, but its error is even in r and has a mean of +4e-17 over the
// interval: summed over n rows at a fit (every t near 0) that is n a 4e-17 in d lp / d alpha, 1.7e-9 at n = 4,097
// and a = 1e4, more than the 1e-9 bar of a small gradient component there (1e-10 x 1e-3 x max |g|, max |g| about 1e4).
// The quartic has no such mean: what is left is the rounding of the table entries and of the fma.
// T overflows to +inf past t = 709.78 and e^t - 1 is then +inf or NaN (inf rr + inf with rr <= 0), and underflows
// to 0 (e^t - 1 = -1).  t itself enters h unclamped: t < -800 gives h = -1 - t, which is h to the last bit; where
// e^t overflows h is +inf or NaN and lp -inf or NaN, never a finite number and never +inf; a NaN eta (the clamp
// turns it into a finite argument) stays NaN in lm through t.
// No reciprocal, no log1p, no running product, no second sum: the lightest residual after Poisson's -- 21 vector
// instructions per element over the linear kernel's by the ISA count of k_sweep16<FAM, 25>, against 14 for Poisson,
// 64 for logistic, 67 for student_t and 74 for the negative binomial counted the same way.
__device__ __forceinline__ double gamma_resid(double eta, double ly, double a, const double* tab, double& lm) {
  constexpr double MAGIC = 6755399441055744.0;            // 1.5 * 2^52
  constexpr double INV_L = 1477.3197218702985;            // 1024 / ln 2
  constexpr double L = 0.0006769015435155716;             // ln 2 / 1024
  const double t = ly - eta;
  const double c = clamp800(t);
  const double sn = fma(c, INV_L, MAGIC);
  const int ni = (int)(uint32_t)__builtin_bit_cast(uint64_t, sn);
  const double n = sn - MAGIC;
  const double r = fma(-n, L, c);
  const double rr = fma(r * r, fma(fma(1.0 / 24.0, r, 1.0 / 6.0), r, 0.5), r);
  const double T = __builtin_amdgcn_ldexp(tab[ni & (EX_TAB - 1)], ni >> 10);
  const double em1 = fma(T, rr, T - 1.0);
  lm += em1 - t;
  return a * em1;
}

// The same terms with libm's expm1, for the VALU sweeps (k_sweep, k_sweep2, k_sweep3: C <= 8), which keep no
// exp table.
__device__ __forceinline__ double gamma_resid_libm(double eta, double ly, double a, double& lm) {
  const double t = ly - eta;
  const double em1 = expm1(t);
  lm += em1 - t;
  return a * em1;
}

// The reduces' chunk order, shared by sweep.hip's and sweep_cat.hip's.
// Wave w's share of column o of chain c's chunk partials: its contiguous range of the G chunks, summed in order,
// 8 loads in flight.
template <int W>
__device__ __forceinline__ double reduce_chunk_range(const SweepArgs& A, int shard, int c, int C, int o, int w) {
  const int per = (A.G + W - 1) / W;
  const int k0 = w * per, k1 = min(A.G, k0 + per);
  const double* src = A.partial + ((size_t)shard * A.Gs * C + c) * A.PW + o;
  const size_t stride = (size_t)C * A.PW;
  double v = 0.0;
  int k = k0;
  for (; k + 8 <= k1; k += 8) {
    double a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = src[(size_t)(k + i) * stride];
#pragma unroll
    for (int i = 0; i < 8; ++i) v += a[i];
  }
  for (; k < k1; ++k) v += src[(size_t)k * stride];
  return v;
}

}  // namespace stk
