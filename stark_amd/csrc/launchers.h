// Host-side launchers and helpers that cross translation units of libstark_hip.so: declared once
// here, included by the capi*.hip units (the callers) and by every file that defines one, so a signature
// that drifts is a compile error instead of a second overload that links and runs.
#pragma once
#include "common.h"
#include "negbin_math.h"
#include <type_traits>

namespace stk {

struct SweepArgs;   // sweep_common.h (device side)

constexpr int CAT_MAX_CHAINS = 16;   // chains of one k_sweep_cat launch: the MFMA's 16 columns (sweep_cat.hip)

// Which regression sweep runs; the numbers are those of tests/golden/sweep_launch.json.
enum SweepKind : int {
  SWEEP_NONE = 0,     // no sweep: the chunk bytes do not fit a buffer descriptor, or (C, d) has no kernel
  SWEEP_V1 = 1,       // k_sweep       any d <= 1024, C <= 8
  SWEEP_V2 = 2,       // k_sweep2      even d <= 128, C <= 8
  SWEEP_V3 = 3,       // k_sweep3      even d <= 104, C <= 4
  SWEEP_16 = 4,       // k_sweep16     C = 16, d <= 128 (sweep16.hip)
  SWEEP_GEMM64 = 5,   // k_qt_swizzle + k_gemm_fwd + k_gemm_bwd, C = 64
  SWEEP_16W = 6,      // k_sweep16w    C = 16, 128 < d <= 1024 (sweep16w.hip)
  SWEEP_SPARSE = 7,   // k_sweep_sp    sparse (padded-row) shards: C <= 16, any d <= 1024 (sweep_sparse.hip); never
                      // chosen by stk_sweep_plan, whose numbers keep their dense meaning
  SWEEP_CAT = 8,      // k_sweep_cat   STK_CATEGORICAL: C <= 16 chains, K - 1 classes' tiles (sweep_cat.hip); never chosen by
                      // stk_sweep_plan either
};

// The kernel and launch shape of one sweep over a shard of n rows: a function of (n, d, C) only,
// so reductions are identical on 1 or N GPUs.  Built by stk_sweep_plan, the one place that reads
// (n, d, C) to choose a kernel; the launchers dispatch on `kind`.  Kind 0 carries no geometry.
struct SweepLaunch {
  SweepKind kind;
  int C, d;
  int T;              // rows per tile
  int G;              // chunks per shard
  size_t lds;         // dynamic LDS bytes per block (kind 5: pass F's; pass B sizes its own)
  int ld;             // kinds 1, 2: row stride of the X tile in LDS, in doubles; kind 7: bytes of the entry stage in LDS;
                      // kind 8: the classes K
  int ring;           // kind 3: ring slots per wave
  int waves;          // kind 6: waves per block (= column slabs); kind 7: private gradient copies per block
  int64_t Rrows;      // kind 5: rows of the residual matrix R per shard (n rounded up to 64)
  size_t ws_bytes;    // kind 5: workspace bytes one shard needs (beta^T image + R); else 0
};

// What a sparse shard adds to its ShardDev (whose x is null): the padded rows (ELL) of its design matrix.  Row r's
// K slots are idx[r K .. r K + K) and val[r K ..): the row's entries by strictly increasing column, then (0, 0.0).
// A side table of the model, handed to the launch as SweepCall::sp: ShardDev and SweepArgs stay as every dense kernel
// was built with.
struct SpShardDev {
  const int32_t* idx;   // [n][K]
  const double* val;    // [n][K]
  int32_t K;            // the shard's longest row (0: an all-zero matrix)
  int32_t pad_;
};

// What one launch adds to its plan: where the data is and which batch of the shard's chains this is.
struct SweepCall {
  const ShardDev* shards;
  const double* q;        // [nshards * Ct][Dp] evaluation points
  double* partial;        // the batch's [nshards][Gs][C][d + 2] partial sums
  const int* req_step;    // nullptr: every shard runs
  int step_id;
  int* ran;               // nullptr, or the profiling counters
  const SweepWs* ws;      // kind 5's workspace (stk_sweep_ws); nullptr when no batch needs one
  int Dp;
  int Gs;                 // partial-sum stride in chunks per shard: the largest G of the batch's groups
  int Ct, c0;             // chains per shard in q / lp / grad, first chain of this batch
  const NbShardDev* nb = nullptr;   // STK_NEGBIN: the model's [nshards] count tables and phi priors (the reduce reads them);
                                    // STK_GAMMA: the shards' L = sum log y and the shape prior, in the same entries
  const SpShardDev* sp = nullptr;   // a sparse model's [nshards] padded rows (kind 7 reads them); else NULL
};

// Columns of a chunk's partial row per chain: d alpha, d beta[1..d], the lp sum -- and the family's third
// sum where it has one (fam_sum3, sweep_common.h).  Defined in sweep.hip.
int sweep_pw(int family, int d);

// The one place a runtime family id becomes a template argument: f(std::integral_constant<int, FAM>) for
// the six regression families, hipErrorInvalidValue for anything else.
template <class F>
hipError_t sweep_family(int family, F&& f) {
  switch (family) {
    case STK_LINREG: return f(std::integral_constant<int, STK_LINREG>());
    case STK_LOGREG: return f(std::integral_constant<int, STK_LOGREG>());
    case STK_POISSON: return f(std::integral_constant<int, STK_POISSON>());
    case STK_NEGBIN: return f(std::integral_constant<int, STK_NEGBIN>());
    case STK_STUDENT: return f(std::integral_constant<int, STK_STUDENT>());
    case STK_GAMMA: return f(std::integral_constant<int, STK_GAMMA>());
  }
  return hipErrorInvalidValue;
}

}  // namespace stk

// ---- sweep.hip
bool stk_sweep_supported(int C, int d);
// force: 1 | 2 pins k_sweep | k_sweep2 where the shape allows (tools/sweep_micro.hip); the library passes 0.
stk::SweepLaunch stk_sweep_plan(int64_t n, int d, int C, int force);
int stk_sweep_args_ld(const stk::SweepLaunch& p);   // the plan's per-kind field as SweepArgs.LD
stk::SweepWs stk_sweep_ws(void* base, const stk::SweepLaunch& at_nmax, int nshards);
hipError_t stk_launch_sweep(int family, const stk::SweepLaunch& p, int shard0, int nsh, const stk::SweepCall& c,
                            hipStream_t st);
hipError_t stk_launch_sweep_reduce(int family, const stk::SweepLaunch& p, int shard0, int nsh, const stk::SweepCall& c,
                                   double* lp_out, double* g_out, hipStream_t st);

// One launcher template per launch point, defined in its kernel file and instantiated in the object that
// holds the family (STK_SWEEP_TU, sweep_common.h): k_sweep / k_sweep2 / k_sweep3, pass F of the 64-chain
// sweep, and the reduce (only the negative binomial's and the gamma family's read nb).
template <int FAM>
hipError_t stk_launch_sweep_valu(const stk::SweepLaunch& p, const stk::SweepArgs& A, int nblocks, hipStream_t st);
template <int FAM>
hipError_t stk_launch_gemm_fwd(const stk::SweepArgs& A, int d, int nblocks, size_t lds, hipStream_t st);
template <int FAM>
hipError_t stk_launch_reduce(const stk::SweepArgs& A, const stk::NbShardDev* nb, int nchains, int d, double* lp_out,
                             double* g_out, int C, hipStream_t st);

// ---- sweep_sparse.hip (sparse shards: C in {1, 2, 4, 8, 16}, 16 up to d = 512; any d <= 1024): the batch sizes it
// covers, its plan (a function of (n, d, C) alone: the chunks of n alone), its launch
bool stk_sweep_sparse_supported(int C, int d);
stk::SweepLaunch stk_sweep_plan_sparse(int64_t n, int d, int C);
hipError_t stk_launch_sweep_sparse(int family, const stk::SweepLaunch& p, int shard0, int nsh, const stk::SweepCall& c,
                                   hipStream_t st);
template <int FAM>
hipError_t stk_launch_sweep_sp(const stk::SweepLaunch& p, const stk::SweepArgs& A, const stk::SpShardDev* sp, int nblocks,
                               hipStream_t st);

// ---- sweep_cat.hip (STK_CATEGORICAL): the envelope in (G = K - 1, d), the plan of one launch of C <= 16 chains (chunks
// of (n, d) alone), the partial row's width G (d + 1) + 1, the sweep, its reduce, and the device check of y in [1, K]
bool stk_sweep_cat_supported(int G, int d);
stk::SweepLaunch stk_sweep_plan_cat(int64_t n, int d, int C, int ncat);
int stk_sweep_cat_pw(int ncat, int d);
hipError_t stk_launch_sweep_cat(const stk::SweepLaunch& p, int shard0, int nsh, const stk::SweepCall& c, hipStream_t st);
hipError_t stk_launch_sweep_reduce_cat(const stk::SweepLaunch& p, int shard0, int nsh, const stk::SweepCall& c, double* lp_out,
                                       double* g_out, hipStream_t st);
hipError_t stk_launch_check_ycat(const int32_t* y, int64_t n, int K, int64_t* first, hipStream_t st);

// ---- sweep16.hip: shapes k_sweep16 covers, its LDS bytes, its launch
bool stk_sweep16_supported(int d);
size_t stk_sweep16_lds_bytes(int family, int d);
template <int FAM>
hipError_t stk_launch_sweep16(const stk::SweepArgs& A, int d, int nblocks, size_t lds, hipStream_t st);

// ---- sweep16w.hip (128 < d <= 1024): waves per block, chunks per shard, LDS bytes, launch
bool stk_sweep16w_supported(int d);
int stk_sweep16w_waves(int d);
int stk_sweep16w_chunks(int64_t n);
size_t stk_sweep16w_lds_bytes(int family, int d);
template <int FAM>
hipError_t stk_launch_sweep16w(const stk::SweepArgs& A, int d, int nblocks, size_t lds, hipStream_t st);

// ---- hessian.hip (regressions, d <= 128): the analytic Hessian sweep's geometry and launch
bool stk_hessian_supported(int d);
int stk_hessian_chunks(int64_t n);
int stk_hessian_rows_per_tile();
int stk_hessian_waves();
size_t stk_hessian_lds_bytes(int d);
size_t stk_hessian_ws_bytes(int64_t n, int d);   // chunk-partial workspace of one shard
hipError_t stk_launch_hessian(int family, const stk::ShardDev* shards, int shard0, int nsh, int d, int D, int Gs,
                              const double* q, double* partial, double* hess, hipStream_t st);

// ---- predictive.hip (regressions, d <= 128): the pointwise log-predictive sweep's geometry and launches
bool stk_predictive_supported(int d);
int stk_predictive_chunks(int64_t n);
int stk_predictive_rows_per_tile();
int stk_predictive_waves();
int stk_predictive_tiles(int S);                   // 16-draw tiles
size_t stk_predictive_lds_bytes(int d);
size_t stk_predictive_image_bytes(int d, int S);
size_t stk_predictive_ws_bytes(int64_t n);         // chunk-partial workspace of one shard
hipError_t stk_launch_predictive_prep(int family, int d, int D, int S, const double* q, double* img, hipStream_t st);
hipError_t stk_launch_predictive(int family, const stk::ShardDev* shards, int shard0, int nsh, int d, int Gs, int S,
                                 const double* img, double* partial, double* rows, const int64_t* rowoff,
                                 double* totals, hipStream_t st);

// ---- loo.hip (regressions, d <= 128, S <= 1024): the PSIS-LOO sweep's geometry and launch; the draw
// image is stk_launch_predictive_prep's
bool stk_loo_supported(int d);
int stk_loo_max_draws();
int stk_loo_chunks(int64_t n);
int stk_loo_rows_per_tile();
int stk_loo_waves(int S);
size_t stk_loo_lds_bytes(int d, int S);
size_t stk_loo_ws_bytes(int64_t n);                // chunk-partial workspace of one shard
hipError_t stk_launch_loo(int family, const stk::ShardDev* shards, int shard0, int nsh, int d, int Gs, int S,
                          const double* img, double* partial, double* rows, const int64_t* rowoff, double* totals,
                          hipStream_t st);

// ---- logdens.hip (regressions, d <= 128, any S): the per-draw log-density sweep's geometry and launch (the
// draw image is stk_launch_predictive_prep's), and the Laplace proposal generator (D <= stk_laplace_max_dim())
bool stk_logdens_supported(int d);
int stk_logdens_chunks(int64_t n);
int stk_logdens_rows_per_tile();
int stk_logdens_waves();
size_t stk_logdens_lds_bytes(int d);
size_t stk_logdens_ws_bytes(int64_t n, int S);     // chunk-partial workspace of one shard
hipError_t stk_launch_logdens(int family, const stk::ShardDev* shards, int shard0, int nsh, int d, int D, int Gs, int S,
                              const double* img, const double* q, double* partial, double* lp, hipStream_t st);
int stk_laplace_max_dim();
hipError_t stk_launch_laplace_draws(const double* mode, const double* factor, int D, int S, uint64_t seed,
                                    uint32_t stream, double* q, double* log_q, hipStream_t st);

// ---- boot.hip (regressions, d <= 128): the weighted bootstrap sweep's geometry and its launch for one tile of
// 16 replicates
bool stk_boot_supported(int d);
int stk_boot_chunks(int64_t n);
int64_t stk_boot_chunk_rows(int64_t n);            // rows of the longest chunk
int stk_boot_rows_per_tile();
int stk_boot_waves();
size_t stk_boot_lds_bytes(int d);
size_t stk_boot_ws_bytes(int64_t n, int d);        // chunk-partial workspace of one shard
hipError_t stk_launch_boot(int family, const stk::ShardDev* shards, int shard0, int nsh, int d, int Gs, int Dp,
                           const double* q, double* partial, const int32_t* streams, uint64_t seed, int rep0, int kind,
                           int R, int c0, int nrep, double* lp, double* grad, double* wsum, hipStream_t st);

// ---- ppc.hip (regressions, d <= 128, any S): the posterior predictive replicate sweep's geometry and launch (the
// draw image is stk_launch_predictive_prep's).  stats [nsh][S][8], obs [nsh][8]; rows ([sum n][4]) and yrep
// ([sum n][S]) may be null; partial holds stk_ppc_ws_bytes of every shard at the stride Gs.
bool stk_ppc_supported(int d);
int stk_ppc_chunks(int64_t n);
int stk_ppc_rows_per_tile();
int stk_ppc_waves();
size_t stk_ppc_lds_bytes(int d);
size_t stk_ppc_ws_bytes(int64_t n, int S);         // chunk-partial workspace of one shard
hipError_t stk_launch_ppc(int family, const stk::ShardDev* shards, int shard0, int nsh, int d, int Gs, int S, int draw0,
                          uint64_t seed, const int32_t* streams, const double* img, double* partial, double* stats,
                          double* obs, double* rows, double* yrep, const int64_t* rowoff, hipStream_t st);

// ---- nuts.hip (and its nuts_fused4.hip / nuts_dense.hip translation units)
int stk_nch_for(int Dmax);
size_t stk_fused_lds_bytes(const stk::NutsArgs& A, int nch);
hipError_t stk_launch_nuts_init(const stk::NutsArgs& A, const double* init, const double* inv_metric, double stepsize,
                                double init_radius, hipStream_t st);
hipError_t stk_launch_nuts_step(const stk::NutsArgs& A, int nch, int step_id, int pause_at, hipStream_t st);
hipError_t stk_launch_nuts_fused(const stk::NutsArgs& A, int nch, int pause_at, int max_steps, hipStream_t st);
hipError_t stk_launch_dense_init(const stk::NutsArgs& A, const double* minv0, const double* chol0, hipStream_t st);
hipError_t stk_launch_nuts_step_dense(const stk::NutsArgs& A, int nch, int step_id, int pause_at, hipStream_t st);
hipError_t stk_launch_schools_lpgrad(const stk::ShardDev* shards, int shard, int nch, const double* q, int C, int Dp,
                                     double* lp, double* g, hipStream_t st);

// ---- datagen.hip
hipError_t stk_launch_check_y01(const int32_t* y, int64_t n, int64_t* first, hipStream_t st);
hipError_t stk_launch_check_ynonneg(const int32_t* y, int64_t n, int64_t* first, hipStream_t st);
hipError_t stk_launch_gen_shard(double* X, double* yd, int32_t* yi, int64_t nrows, int d, int64_t grow0,
                                uint64_t seed, double alpha, const double* beta, double noise_sigma, int family,
                                hipStream_t st);

// ---- combine.hip
hipError_t stk_launch_consensus_products(const double* X, int nshards, int P, int S, const int32_t* blk, double* mean,
                                         int32_t* rowbad, int32_t* used, int32_t* status, double* cov, double* W,
                                         double* work, double* sum_w, double* sum_wtheta, hipStream_t st);
size_t stk_general_inverse_work_bytes(int P);
hipError_t stk_launch_consensus_solve(const double* sum_w, const double* sum_wtheta, int P, int S, double* inv_buf,
                                      double* work, int32_t* status, double* out, hipStream_t st, bool general);
size_t stk_spd_inverse_work_bytes(int P, int batch);
hipError_t stk_launch_spd_inverse(const double* M, double* Inv, double* work, int P, int batch, const int32_t* used,
                                  int32_t* status, hipStream_t st);
// the caller's weights W [nshards][P][P] (device, modified: NaN-draw shards are zeroed) in place of inv(cov)
hipError_t stk_launch_consensus_weighted(const double* X, int nshards, int P, int S, double* mean, int32_t* rowbad,
                                         int32_t* used, int32_t* status, double* W, double* sum_w, double* sum_wtheta,
                                         hipStream_t st);

// ---- dpe.hip: the semiparametric density-product combiner (kernels and the host twin of the chains)
struct StkDpeChains {
  const double *Y, *nrm, *g, *lpv, *lpw;   // the prepared arrays of the M usable shards; lpv / lpw null: no lp__ row
  const void* coef;                        // [sweeps] stk::DpeCoef (dpe_math.h)
  double* ydraw;                           // device: [T][ldp] whitened draws
  double* lpout;                           // device: [T] the lp__ row, or null
  unsigned long long* accept;              // [M], added to
  int32_t* tidx;                           // [K][sweeps][M] or null
  double* tlogw;                           // [K][sweeps] or null
  uint64_t seed;
  uint32_t stream;
  int M, p, S, T, K, burn, thin, sweeps;
};
int stk_dpe_coords_per_lane(int p);
size_t stk_dpe_lds_bytes(int M);
hipError_t stk_launch_dpe_image(const double* X, const double* mean, const double* W, const int32_t* zmap, int M, int P,
                                int p, int S, const double* mu, const double* Linv, double* Y, double* Z, double* nrm,
                                double* g, double* lpv, hipStream_t st);
hipError_t stk_launch_dpe_chains(const StkDpeChains& c, hipStream_t st);
hipError_t stk_launch_dpe_map(const double* ydraw, const double* L, const double* mu, int M, int p, int T, double* out,
                              hipStream_t st);
void stk_dpe_chains_host(const StkDpeChains& c, const double* mu, const double* L, double* out);

// ---- fingerprint.hip
uint64_t stk_fp_fmix(uint64_t a);
uint64_t stk_fp_words_host(const void* buf, int64_t count, int word_bytes, int tag, uint64_t index0);
hipError_t stk_launch_fp_words(const void* buf, int64_t count, int word_bytes, int tag, uint64_t index0,
                               unsigned long long* sum, hipStream_t st);
